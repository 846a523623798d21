# CPU restatement of grassfire, the blob index, ErodeView, InpaintView, fill_holes_grass and fill_nodata_with_avg
# (test infrastructure only); make -f hole_fill_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libhole_fill_ref.so

libhole_fill_ref.so: hole_fill_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ hole_fill_ref.cc -pthread

clean:
	rm -f libhole_fill_ref.so
