# CPU restatement of epipolar rectification (epipolar(), the camera matrix, CameraTransform and camera_transform over
# bilinear interpolation; test infrastructure only); make -f epipolar_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libepipolar_ref.so

libepipolar_ref.so: epipolar_ref.cc triangulate_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ epipolar_ref.cc

clean:
	rm -f libepipolar_ref.so
