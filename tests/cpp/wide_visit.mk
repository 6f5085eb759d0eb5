# TEST PROGRAM build: the device's wide_visit on dumped (node, ray) pairs (wide_visit_units.hip, for
# tests/test_gpu_wide_visit.py), compiled with the library's numeric and device flags.
#   make -C tests/cpp -f wide_visit.mk
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
BUILD := _build
CSRC  := ../../simplepath_amd/csrc
include ../../simplepath_amd/flags.mk

$(BUILD)/wide_visit_units: wide_visit_units.hip $(wildcard $(CSRC)/common/*.h $(CSRC)/hip/*.hpp ../../include/*.h) ../../simplepath_amd/flags.mk
	@mkdir -p $(BUILD)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable $(NUMFLAGS) $(HIPFLAGS) -I$(CSRC)/hip $< -o $@
