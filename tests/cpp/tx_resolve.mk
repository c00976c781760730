# Tx resolve: the shared decision, record and header stores (aipstack_amd/csrc/txres_common.h) and
# the host code (txres_host.cpp, plain C++ without a HIP call) in a stand-alone test under
# AddressSanitizer + UBSan.
#   make -C tests/cpp -f tx_resolve.mk        build/asan/tx_resolve_build_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/tx_resolve_build_test

build/asan/tx_resolve_build_test: tx_resolve_build_test.cpp $(CSRC)/txres_host.cpp $(CSRC)/txres_common.h \
                                  $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ tx_resolve_build_test.cpp $(CSRC)/txres_host.cpp

.PHONY: all
