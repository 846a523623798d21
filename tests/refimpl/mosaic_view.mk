# mosaic_view: a vwlite program over libvwgpu.so (test infrastructure only); make -f mosaic_view.mk.
CXX ?= g++
ROOT := ../..
LIBDIR := $(abspath $(ROOT)/visionworkbench_amd/lib)
ROCM_LIB ?= /opt/rocm/lib
CXXFLAGS ?= -O1 -std=c++17 -Wall -ffp-contract=off

all: mosaic_view

mosaic_view: mosaic_view.cc $(ROOT)/visionworkbench_amd/vwlite/vw/Mosaic.h $(ROOT)/visionworkbench_amd/vwlite/vw/Image.h $(ROOT)/include/vwgpu.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -I$(ROOT)/visionworkbench_amd/vwlite -o $@ mosaic_view.cc -L$(LIBDIR) -lvwgpu -Wl,-rpath,$(LIBDIR) -Wl,-rpath,$(ROCM_LIB) -pthread

clean:
	rm -f mosaic_view
