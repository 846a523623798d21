# CPU restatement of two-camera triangulation (StereoModel, StereoView, UniverseRadiusFunc and the pinhole / Tsai / CAHV
# rays they need; test infrastructure only); make -f triangulate_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libtriangulate_ref.so

libtriangulate_ref.so: triangulate_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ triangulate_ref.cc

clean:
	rm -f libtriangulate_ref.so
