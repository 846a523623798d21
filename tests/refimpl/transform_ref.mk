# CPU restatement of vw::transform for the closed-form 2-D maps (the map functors, the edge extensions, the three
# interpolations, TransformView and TransformViewNoData; test infrastructure only); make -f transform_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libtransform_ref.so

libtransform_ref.so: transform_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ transform_ref.cc

clean:
	rm -f libtransform_ref.so
