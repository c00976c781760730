# ARP on receive: the shared record and reply builder (aipstack_amd/csrc/arp_common.h) and the
# host code (arp_host.cpp, plain C++ without a HIP call) in a stand-alone test under
# AddressSanitizer + UBSan.
#   make -C tests/cpp -f arp.mk        build/asan/arp_build_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/arp_build_test

build/asan/arp_build_test: arp_build_test.cpp $(CSRC)/arp_host.cpp $(CSRC)/arp_common.h \
                           $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ arp_build_test.cpp $(CSRC)/arp_host.cpp

.PHONY: all
