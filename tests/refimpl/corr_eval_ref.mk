# CPU restatement of vw::stereo::corr_eval (CorrEval::prerasterize; test infrastructure only); make -f corr_eval_ref.mk.
# Same numerics flags as the oracle (no FMA contraction, no fast-math).
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra

all: libcorr_eval_ref.so

libcorr_eval_ref.so: corr_eval_ref.cc
	$(CXX) $(CXXFLAGS) -shared -o $@ corr_eval_ref.cc -pthread

clean:
	rm -f libcorr_eval_ref.so
