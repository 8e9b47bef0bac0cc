# CPU only, like sanitize.mk, whose variables and object rules it uses (through the Makefile): the per-lane pairing checks
# (csrc/pairing_device.h, csrc/pairing_tower.h) as a stand-alone program under AddressSanitizer AND UBSan, with its own main —
# nothing is loaded into Python, no LD_PRELOAD.  plonk_pairing_check_many on true and false checks, identities and a second
# workgroup against the host's plonk_pairing_check; the refused arguments.      make -C tests/emu -f pairing_sanitize.mk -j8 pairing-sanitize
include Makefile
ifndef SAN_BOTH
$(error sanitize.mk is not here: its flags and object rules are what this target is built with)
endif
asan/pairing_sanitize: $(SRCS:$(CSRC)/%.hip=asan/intake/%.o) asan/intake/hip_emu.o asan/intake/comm_stub.o asan/intake/pairing_sanitize.o
	$(CXX) $(SAN_BOTH) -o $@ $^
pairing-sanitize: asan/pairing_sanitize
	ASAN_OPTIONS=detect_stack_use_after_return=0 ./asan/pairing_sanitize
.PHONY: pairing-sanitize
