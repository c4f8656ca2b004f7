// global_bytes.h - how the 8-bit kernels (ingest.hip, facemask.hip) name global memory and take bytes out of loaded dwords.  Device
// code only.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "resize_taps.h"

// a descriptor's pointers are global memory: said so, the loads and stores are global_* instead of flat_* instructions
#define RTD_GLOBAL __attribute__((address_space(1)))
typedef const RTD_GLOBAL uint8_t* GBytes;
typedef const RTD_GLOBAL uint16_t* GHalf;
typedef const RTD_GLOBAL uint32_t* GWord;
typedef const RTD_GLOBAL int32_t* GInt;
typedef const RTD_GLOBAL resize_taps::LinEntry* GLin;
typedef RTD_GLOBAL uint8_t* GOut;
typedef RTD_GLOBAL uint16_t* GOutHalf;
typedef RTD_GLOBAL uint32_t* GOutWord;

// byte i of the little-endian dwords w[]
__device__ inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }
