# CPU only, like sanitize.mk, whose variables and object rules it uses (through the Makefile): the witness solver's plan
# (csrc/witness_solve.h) as a stand-alone program under AddressSanitizer AND UBSan, with its own main — nothing is loaded into
# Python, no LD_PRELOAD.  Descriptors and the levelised form's schedule across two plans, a new wiring, uploads under both forms,
# a prover destroyed with a plan and no upload.      make -C tests/emu -f levels_sanitize.mk -j8 levels-sanitize
include Makefile
ifndef SAN_BOTH
$(error sanitize.mk is not here: its flags and object rules are what this target is built with)
endif
asan/levels_lifetime: $(SRCS:$(CSRC)/%.hip=asan/intake/%.o) asan/intake/hip_emu.o asan/intake/comm_stub.o asan/intake/levels_lifetime.o
	$(CXX) $(SAN_BOTH) -o $@ $^
levels-sanitize: asan/levels_lifetime
	ASAN_OPTIONS=detect_stack_use_after_return=0 ./asan/levels_lifetime
.PHONY: levels-sanitize
