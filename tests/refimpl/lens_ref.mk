# CPU restatement of the FOV, fisheye, Brown-Conrady, adjustable Tsai and Photometrix lens distortions, the pinhole around
# them and its camera-transform and triangulation compositions (test infrastructure only); make -f lens_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: liblens_ref.so

liblens_ref.so: lens_ref.cc epipolar_ref.cc triangulate_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ lens_ref.cc

clean:
	rm -f liblens_ref.so
