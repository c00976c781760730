# UDP Rx demux: the shared record builder, listener match (aipstack_amd/csrc/udprx_common.h) and
# table search (pcb_lookup.h) and the host code (udprx_host.cpp, plain C++ without a HIP call) in
# a stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f udprx.mk        build/asan/udprx_table_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/udprx_table_test

build/asan/udprx_table_test: udprx_table_test.cpp $(CSRC)/udprx_host.cpp $(CSRC)/udprx_common.h \
                             $(CSRC)/pcb_lookup.h $(CSRC)/tcprx_common.h $(CSRC)/icmp_common.h \
                             $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ udprx_table_test.cpp $(CSRC)/udprx_host.cpp

.PHONY: all
