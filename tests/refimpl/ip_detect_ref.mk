# CPU restatement of the OBALoG detectors and the SGrad descriptors (IntegralImage, the interest planes, extrema, threshold and
# Harris, order and cull, orientation, SGrad, SGrad2; test infrastructure only); make -f ip_detect_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libip_detect_ref.so

libip_detect_ref.so: ip_detect_ref.cc ../../visionworkbench_amd/csrc/ip_atan2.h ../../visionworkbench_amd/csrc/ip_obalog.h
	$(CXX) $(CXXFLAGS) -shared -o $@ ip_detect_ref.cc

clean:
	rm -f libip_detect_ref.so
