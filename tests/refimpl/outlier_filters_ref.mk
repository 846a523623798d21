# CPU restatement of the local outlier filters of Stereo/DisparityMap.h (mean, stddev, plane, their clean-up
# compositions) and std_dev_image (test infrastructure only); make -f outlier_filters_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: liboutlier_filters_ref.so

liboutlier_filters_ref.so: outlier_filters_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ outlier_filters_ref.cc -pthread

clean:
	rm -f liboutlier_filters_ref.so
