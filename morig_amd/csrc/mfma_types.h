// The register and pointer types of the MFMA kernels, stated once: the accumulator tile of v_mfma_f32_32x32x16_*, its 4-register
// groups, the fp16 / bf16 operand fragments (8 halves = one ds_read_b128), and the address-space pointers __builtin_amdgcn_global_load_lds
// takes. Included by common.h, so every translation unit and the epilogue headers see the same names.
#pragma once

namespace morig {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

}  // namespace morig
