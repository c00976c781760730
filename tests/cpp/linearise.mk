# Linearising header-split Tx segments: the shared rule and piece lookup
# (aipstack_amd/csrc/linearise_common.h) and the host checks (linearise_host.cpp, plain C++
# without a HIP call) in a stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f linearise.mk        build/asan/linearise_plan_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/linearise_plan_test

build/asan/linearise_plan_test: linearise_plan_test.cpp $(CSRC)/linearise_host.cpp \
                                $(CSRC)/linearise_common.h $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ linearise_plan_test.cpp $(CSRC)/linearise_host.cpp

.PHONY: all
