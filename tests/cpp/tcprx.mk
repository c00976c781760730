# TCP Rx parse: the host code (aipstack_amd/csrc/tcprx_host.cpp, plain C++ without a HIP call)
# and its stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f tcprx.mk        build/asan/tcprx_table_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/tcprx_table_test

build/asan/tcprx_table_test: tcprx_table_test.cpp $(CSRC)/tcprx_host.cpp $(CSRC)/tcprx_common.h \
                             $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ tcprx_table_test.cpp $(CSRC)/tcprx_host.cpp

.PHONY: all
