# Sanitizer builds of the emulated kernels: CPU only (g++ or clang++ on the host emulation of the kernel sources).  Included by
# tests/emu/Makefile when present; listed in .gpurunignore — sanitizers are not run on the GPU pool, and nothing a GPU box
# runs needs these recipes.
# AddressSanitizer build of the emulated kernels (heap out-of-bounds reads / writes of device buffers and LDS in any kernel),
# compiled by clang with GPU sanitizing switched off explicitly (-fno-gpu-sanitize): the sources are compiled as host C++ only:
#   make -C tests/emu asan && cp tests/emu/asan/libplonk_emu.so tests/emu/ && \
#   LD_PRELOAD=$(clang++ -print-file-name=libclang_rt.asan-x86_64.so) ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 \
#     python -m pytest tests/test_emu_parity.py tests/test_distributed_gloo.py tests/test_bench_cli.py ; make -C tests/emu clean all
# (ucontext fibers: ASan prints one "doesn't fully support swapcontext" warning; round 2's final sources pass clean.
#  The same recipe with -fsanitize=signed-integer-overflow,bounds and libubsan.so checks the signed-limb arithmetic.)
asan:
	@mkdir -p asan
	$(MAKE) -s BUILD_ASAN=1 asan/libplonk_emu.so
ASAN_CXX ?= clang++
asan/libplonk_emu.so: $(SRCS) hip_emu.cpp comm_stub.cpp $(HDRS)
	for f in $(SRCS); do $(ASAN_CXX) $(CXXFLAGS) -O1 -g -fno-gpu-sanitize -fsanitize=address -fno-omit-frame-pointer -x c++ -c $$f -o asan/$$(basename $$f .hip).o || exit 1; done
	$(ASAN_CXX) $(CXXFLAGS) -O1 -g -fno-gpu-sanitize -fsanitize=address -fno-omit-frame-pointer -c hip_emu.cpp -o asan/hip_emu.o
	$(ASAN_CXX) $(CXXFLAGS) -O1 -g -fno-gpu-sanitize -fsanitize=address -fno-omit-frame-pointer -c comm_stub.cpp -o asan/comm_stub.o
	$(ASAN_CXX) -shared -fno-gpu-sanitize -fsanitize=address -o $@ asan/*.o

# the same with UBSan (signed overflow of the limb arithmetic, array bounds):  make -C tests/emu ubsan && cp tests/emu/ubsan/libplonk_emu.so tests/emu/ &&
#   LD_PRELOAD=$(gcc -print-file-name=libubsan.so) python -m pytest tests/test_emu_parity.py ; make -C tests/emu clean all
UBSAN := -fsanitize=signed-integer-overflow,bounds -fno-sanitize-recover=signed-integer-overflow,bounds
ubsan:
	@mkdir -p ubsan
	for f in $(SRCS); do $(CXX) $(CXXFLAGS) -O1 -g $(UBSAN) -x c++ -c $$f -o ubsan/$$(basename $$f .hip).o || exit 1; done
	$(CXX) $(CXXFLAGS) -O1 -g $(UBSAN) -c hip_emu.cpp -o ubsan/hip_emu.o
	$(CXX) $(CXXFLAGS) -O1 -g $(UBSAN) -c comm_stub.cpp -o ubsan/comm_stub.o
	$(CXX) -shared $(UBSAN) -o ubsan/libplonk_emu.so ubsan/*.o

# A stand-alone program under AddressSanitizer AND UBSan, with its own main (nothing is loaded into Python, no LD_PRELOAD): the
# prover's intake (csrc/prover_intake.h) — buffers and events across batches of 2, 5 and 1 through every kind of upload, a second
# plan, a prover destroyed without an upload.      make -C tests/emu -j8 intake-sanitize
SAN_BOTH := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
asan/intake/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p asan/intake
	$(CXX) $(CXXFLAGS) $(SAN_BOTH) -x c++ -c $< -o $@
asan/intake/%.o: %.cpp $(HDRS)
	@mkdir -p asan/intake
	$(CXX) $(CXXFLAGS) $(SAN_BOTH) -I../../include -c $< -o $@
asan/intake_lifetime: $(SRCS:$(CSRC)/%.hip=asan/intake/%.o) asan/intake/hip_emu.o asan/intake/comm_stub.o asan/intake/intake_lifetime.o
	$(CXX) $(SAN_BOTH) -o $@ $^
intake-sanitize: asan/intake_lifetime
	ASAN_OPTIONS=detect_stack_use_after_return=0 ./asan/intake_lifetime
.PHONY: intake-sanitize
