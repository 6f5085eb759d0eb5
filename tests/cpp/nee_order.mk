# TEST PROGRAM build: direct_nee beside the order it replaced (nee_order_units.hip, for
# tests/test_gpu_nee_order.py), compiled with the library's numeric and device flags, once per form
# of SP_NEE_SKIP (0: never skip, 1: the wave vote, 2: each lane on its own -- the library's default).
#   make -C tests/cpp -f nee_order.mk
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
BUILD := _build
CSRC  := ../../simplepath_amd/csrc
include ../../simplepath_amd/flags.mk

all: $(BUILD)/nee_order_units_0 $(BUILD)/nee_order_units_1 $(BUILD)/nee_order_units_2

$(BUILD)/nee_order_units_%: nee_order_units.hip $(wildcard $(CSRC)/common/*.h $(CSRC)/hip/*.hpp ../../include/*.h) ../../simplepath_amd/flags.mk
	@mkdir -p $(BUILD)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable $(NUMFLAGS) $(HIPFLAGS) -DSP_NEE_SKIP=$* -I$(CSRC)/hip $< -o $@
.PHONY: all
