// zhip_device_emu_wave.hpp -- the host wave emulator's form of the primitive the wave match finder adds to python-zstandard_amd/csrc/zhip_device.hpp
// (test infrastructure beside tests/emu/emu_wave_finder.cpp; included after zhip_device.hpp's emulator half, before zhip_encode_wave.hpp).
#pragma once
// lanes are fibers that run one at a time between two rendezvous: a plain read-modify-write is atomic here
ZH_DEV void zh_lds_atomic_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
