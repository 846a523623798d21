# CPU restatement of the image statistics and intensity scaling of Image/Statistics.h, ImageThresh.h, Algorithms.h and
# AutoNormalize.h (test infrastructure only); make -f image_stats_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libimage_stats_ref.so

libimage_stats_ref.so: image_stats_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ image_stats_ref.cc -pthread

clean:
	rm -f libimage_stats_ref.so
