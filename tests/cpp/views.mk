# TEST PROGRAM build: camera edits and many views in one launch through the C++ drop-in header
# (views_main.cpp, for tests/test_gpu_views.py), linked against the in-tree library like a host would.
#   make -C tests/cpp -f views.mk
CXX   ?= g++
BUILD := _build
LIBDIR := $(abspath ../../simplepath_amd/_build)

all: $(BUILD)/views_main

$(BUILD)/views_main: views_main.cpp ../../include/simplepath_amd.hpp ../../include/simplepath_hip.h $(LIBDIR)/libsimplepath_hip.so
	@mkdir -p $(BUILD)
	$(CXX) -std=c++17 -O2 -Wall -Wextra -I../../include $< -o $@ -L$(LIBDIR) -lsimplepath_hip -Wl,-rpath,'$$ORIGIN/../../../simplepath_amd/_build'
.PHONY: all
