# CPU restatement of phase_subpixel (PyramidSubpixelView with SUBPIXEL_PHASE; test infrastructure only); make -f phase_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math); the fma chains are explicit std::fma calls.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra
ORACLE := ../../oracle

all: libphase_ref.so

$(ORACLE)/libvw_oracle.so:
	$(MAKE) -s -C $(ORACLE)

libphase_ref.so: phase_ref.cc affine_ref.cc tile_range.h $(ORACLE)/vw_oracle.h $(ORACLE)/libvw_oracle.so
	$(CXX) $(CXXFLAGS) -shared -o $@ phase_ref.cc -L$(ORACLE) -lvw_oracle -Wl,-rpath,'$$ORIGIN/../../oracle' -pthread

clean:
	rm -f libphase_ref.so
