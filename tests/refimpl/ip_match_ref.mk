# CPU restatement of the interest-point matchers (InterestPointMatcherSimple, InterestPointMatcher with an exact search,
# the two metrics, the constraints, remove_duplicates; test infrastructure only); make -f ip_match_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libip_match_ref.so

libip_match_ref.so: ip_match_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ ip_match_ref.cc

clean:
	rm -f libip_match_ref.so
