# lens_view: a vwlite program over libvwgpu.so (test infrastructure only); make -f lens_view.mk.
CXX ?= g++
ROOT := ../..
LIBDIR := $(abspath $(ROOT)/visionworkbench_amd/lib)
ROCM_LIB ?= /opt/rocm/lib
CXXFLAGS ?= -O1 -std=c++17 -Wall -ffp-contract=off

all: lens_view

lens_view: lens_view.cc $(ROOT)/visionworkbench_amd/vwlite/vw/Camera.h $(ROOT)/include/vwgpu.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -I$(ROOT)/visionworkbench_amd/vwlite -o $@ lens_view.cc -L$(LIBDIR) -lvwgpu -Wl,-rpath,$(LIBDIR) -Wl,-rpath,$(ROCM_LIB) -pthread

clean:
	rm -f lens_view
