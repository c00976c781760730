# ICMP responder: the shared decision and slot builder (aipstack_amd/csrc/icmp_common.h) and the
# host code (icmp_host.cpp, plain C++ without a HIP call) in a stand-alone test under
# AddressSanitizer + UBSan.
#   make -C tests/cpp -f icmp.mk        build/asan/icmp_build_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/icmp_build_test

build/asan/icmp_build_test: icmp_build_test.cpp $(CSRC)/icmp_host.cpp $(CSRC)/icmp_common.h \
                            $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ icmp_build_test.cpp $(CSRC)/icmp_host.cpp

.PHONY: all
