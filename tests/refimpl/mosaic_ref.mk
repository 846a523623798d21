# CPU restatement of vw::mosaic::ImageComposite (test infrastructure only); make -f mosaic_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libmosaic_ref.so

libmosaic_ref.so: mosaic_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ mosaic_ref.cc

clean:
	rm -f libmosaic_ref.so
