# IPv4 reassembly on receive: the text the host code and the kernels share
# (aipstack_amd/csrc/ipreass_common.h, ipreass_host.cpp; plain C++ without a HIP call) run serially
# by a stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f ipreass.mk        build/asan/ipreass_table_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/ipreass_table_test

build/asan/ipreass_table_test: ipreass_table_test.cpp $(CSRC)/ipreass_host.cpp $(CSRC)/ipreass_common.h \
                               $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ ipreass_table_test.cpp $(CSRC)/ipreass_host.cpp

.PHONY: all
