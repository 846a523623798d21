# CPU restatement of PyramidSubpixelView with LUCAS_KANADE and BAYES_EM (test infrastructure only); make -f pyr_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math); exp is the host libm's.
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra
ORACLE := ../../oracle

all: libpyr_ref.so

$(ORACLE)/libvw_oracle.so:
	$(MAKE) -s -C $(ORACLE)

libpyr_ref.so: pyr_ref.cc affine_ref.cc tile_range.h $(ORACLE)/vw_oracle.h $(ORACLE)/libvw_oracle.so
	$(CXX) $(CXXFLAGS) -shared -o $@ pyr_ref.cc -L$(ORACLE) -lvw_oracle -Wl,-rpath,'$$ORIGIN/../../oracle'

clean:
	rm -f libpyr_ref.so
