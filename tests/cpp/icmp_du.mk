# Received ICMP Destination Unreachable: the shared decision and record builder
# (aipstack_amd/csrc/icmpdu_common.h, on icmp_common.h and pcb_lookup.h) and the host code
# (icmpdu_host.cpp, plain C++ without a HIP call) in a stand-alone test under AddressSanitizer +
# UBSan.
#   make -C tests/cpp -f icmp_du.mk        build/asan/icmp_du_build_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/icmp_du_build_test

build/asan/icmp_du_build_test: icmp_du_build_test.cpp $(CSRC)/icmpdu_host.cpp $(CSRC)/icmpdu_common.h \
                               $(CSRC)/icmp_common.h $(CSRC)/pcb_lookup.h $(CSRC)/tcprx_common.h \
                               $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ icmp_du_build_test.cpp $(CSRC)/icmpdu_host.cpp

.PHONY: all
