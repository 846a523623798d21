# image_stats_view: the C++ surface of the image statistics and intensity scaling (vwlite vw/Image.h, vw/Math.h) on libvwgpu.so, as a
# stand-alone program (test infrastructure only); make -f image_stats_view.mk.
CXX ?= g++
ROOT := ../..
LIBDIR := $(ROOT)/visionworkbench_amd/lib
CXXFLAGS ?= -O1 -std=c++17 -Wall -ffp-contract=off
VWLITE := $(ROOT)/visionworkbench_amd/vwlite

all: image_stats_view

image_stats_view: image_stats_view.cc $(wildcard $(VWLITE)/vw/*.h) $(ROOT)/include/vwgpu.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -I$(VWLITE) -o $@ image_stats_view.cc -L$(LIBDIR) -lvwgpu -Wl,-rpath,$(abspath $(LIBDIR)) -Wl,-rpath,/opt/rocm/lib -pthread

clean:
	rm -f image_stats_view
