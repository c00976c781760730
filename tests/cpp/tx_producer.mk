# The Tx producers' owner search (aipstack_amd/csrc/tx_producer_common.h, plain C++) and its
# stand-alone test under AddressSanitizer + UBSan.
#   make -C tests/cpp -f tx_producer.mk        build/asan/tx_producer_test
ROCM    ?= /opt/rocm
ROOT    := ../..
CSRC    := $(ROOT)/aipstack_amd/csrc
CLANGXX := $(ROCM)/lib/llvm/bin/clang++
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined

all: build/asan/tx_producer_test

build/asan/tx_producer_test: tx_producer_test.cpp $(CSRC)/tx_producer_common.h \
                             $(ROOT)/include/aipstack_amd/chksum.h
	@mkdir -p build/asan
	$(CLANGXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -Wall -Wextra $(SAN) -I$(ROOT)/include -I$(CSRC) \
	    -o $@ tx_producer_test.cpp

.PHONY: all
