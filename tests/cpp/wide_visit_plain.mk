# TEST PROGRAM build: the plain node visit and the walks that vote for it (wide_visit_plain_units.hip,
# for tests/test_gpu_wide_visit_plain.py), compiled with the library's numeric and device flags, once
# per value of SP_VISIT_PLAIN (1: the library's default; 0: every walk visits with spw::visit).
#   make -C tests/cpp -f wide_visit_plain.mk
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
BUILD := _build
CSRC  := ../../simplepath_amd/csrc
include ../../simplepath_amd/flags.mk

all: $(BUILD)/wide_visit_plain_units_0 $(BUILD)/wide_visit_plain_units_1

$(BUILD)/wide_visit_plain_units_%: wide_visit_plain_units.hip $(wildcard $(CSRC)/common/*.h $(CSRC)/hip/*.hpp ../../include/*.h) ../../simplepath_amd/flags.mk
	@mkdir -p $(BUILD)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable $(NUMFLAGS) $(HIPFLAGS) -DSP_VISIT_PLAIN=$* -I$(CSRC)/hip $< -o $@
.PHONY: all
