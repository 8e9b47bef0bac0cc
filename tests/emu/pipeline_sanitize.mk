# CPU only, like sanitize.mk, whose variables and object rules it uses (through the Makefile): the two-slot intake
# (csrc/prover_intake.h: stage, advance) as a stand-alone program under AddressSanitizer AND UBSan, with its own main — nothing is
# loaded into Python, no LD_PRELOAD.  Batches staged and advanced, a larger one staged, a plain upload in between, a new plan with
# nothing staged, a prover destroyed with a batch staged.      make -C tests/emu -f pipeline_sanitize.mk -j8 pipeline-sanitize
include Makefile
ifndef SAN_BOTH
$(error sanitize.mk is not here: its flags and object rules are what this target is built with)
endif
asan/pipeline_lifetime: $(SRCS:$(CSRC)/%.hip=asan/intake/%.o) asan/intake/hip_emu.o asan/intake/comm_stub.o asan/intake/pipeline_lifetime.o
	$(CXX) $(SAN_BOTH) -o $@ $^
pipeline-sanitize: asan/pipeline_lifetime
	ASAN_OPTIONS=detect_stack_use_after_return=0 ./asan/pipeline_lifetime
.PHONY: pipeline-sanitize
