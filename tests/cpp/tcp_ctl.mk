# TCP segments without data: the shared validity rule and builder
# (aipstack_amd/csrc/tcpctl_common.h, on tcprsp_common.h and tcprx_common.h) and the host code
# (tcpctl_host.cpp, plain C++ without a HIP call) in a stand-alone test under AddressSanitizer +
# UBSan.
#   make -C tests/cpp -f tcp_ctl.mk        build/asan/tcp_ctl_build_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/tcp_ctl_build_test

build/asan/tcp_ctl_build_test: tcp_ctl_build_test.cpp $(CSRC)/tcpctl_host.cpp $(CSRC)/tcpctl_common.h \
                               $(CSRC)/tcprsp_common.h $(CSRC)/tcprx_common.h $(CSRC)/icmp_common.h \
                               $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ tcp_ctl_build_test.cpp $(CSRC)/tcpctl_host.cpp

.PHONY: all
