# TEST INFRASTRUCTURE ONLY, with the Makefile's compiler, flags and header list: the host probe of the pairing tower
# (pairing_probe.cpp: csrc/pairing_tower.h and the generated constants for tests/test_emu_pairing_device.py).
#   make -C tests/emu -f pairing_probe.mk libpairing_probe.so
include Makefile
libpairing_probe.so: pairing_probe.cpp hip_emu.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@ pairing_probe.cpp hip_emu.cpp
