# ip_detect_view: the C++ surface of vw::ip detection and description (vwlite vw/InterestPoint.h) on libvwgpu.so, as a stand-alone
# program (test infrastructure only); make -f ip_detect_view.mk.
CXX ?= g++
ROOT := ../..
LIBDIR := $(ROOT)/visionworkbench_amd/lib
CXXFLAGS ?= -O1 -std=c++17 -Wall -ffp-contract=off
VWLITE := $(ROOT)/visionworkbench_amd/vwlite

all: ip_detect_view

ip_detect_view: ip_detect_view.cc $(wildcard $(VWLITE)/vw/*.h) $(ROOT)/include/vwgpu.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/include -I$(VWLITE) -o $@ ip_detect_view.cc -L$(LIBDIR) -lvwgpu -Wl,-rpath,$(abspath $(LIBDIR)) -Wl,-rpath,/opt/rocm/lib -pthread

clean:
	rm -f ip_detect_view
