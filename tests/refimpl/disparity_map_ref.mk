# CPU restatement of the operators of Stereo/DisparityMap.h on a finished disparity map (range, range mask, transforms,
# sub- and upsampling, the DisparityTransform warp, missing_pixel_image, intersect_mask_and_data; test infrastructure
# only); make -f disparity_map_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libdisparity_map_ref.so

libdisparity_map_ref.so: disparity_map_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ disparity_map_ref.cc -pthread

clean:
	rm -f libdisparity_map_ref.so
