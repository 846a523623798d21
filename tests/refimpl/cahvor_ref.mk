# CPU restatement of the CAHVOR and CAHVORE camera models, linearize_camera and their camera-transform and triangulation
# compositions (test infrastructure only); make -f cahvor_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libcahvor_ref.so

libcahvor_ref.so: cahvor_ref.cc epipolar_ref.cc triangulate_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ cahvor_ref.cc

clean:
	rm -f libcahvor_ref.so
