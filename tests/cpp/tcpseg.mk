# TCP burst segmentation: the host code (aipstack_amd/csrc/tcpseg_host.cpp, plain C++ without a
# HIP call) and its stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f tcpseg.mk        build/asan/tcpseg_layout_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/tcpseg_layout_test

build/asan/tcpseg_layout_test: tcpseg_layout_test.cpp $(CSRC)/tcpseg_host.cpp $(CSRC)/tcpseg_common.h \
                               $(CSRC)/tx_producer_common.h \
                               $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ tcpseg_layout_test.cpp $(CSRC)/tcpseg_host.cpp

.PHONY: all
