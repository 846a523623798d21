# CPU restatement of the disparity post-filters of Stereo/Algorithms.h (median, neighbour, texture measure,
# texture-preserving smoothing; test infrastructure only); make -f disparity_filters_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libdisparity_filters_ref.so

libdisparity_filters_ref.so: disparity_filters_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ disparity_filters_ref.cc -pthread

clean:
	rm -f libdisparity_filters_ref.so
