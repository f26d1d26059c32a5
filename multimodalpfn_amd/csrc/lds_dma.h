// The one LDS-DMA issue of the kernels that fill LDS rings without staging registers (gemm.hip, modality.hip,
// attention_pipe.hip, mlp_rows.hip, featrow.hip).
//
// One wave-instruction copies 1 KB: lane i's 16 B land at LDS address m0 + 16 i, m0 being the wave's (scalar) LDS
// destination.  Two contracts come with it:
//  * m0.  The asm writes m0 itself.  clang keeps m0 reserved and ignores the "m0" entry of the clobber list
//    (-Winline-asm, silenced here; the ISA is identical with and without the entry), so nothing stops the compiler
//    from assuming a value of its own survives the asm.  Every m0 use the compiler emits itself is preceded by its
//    own write; tests/test_codegen.py checks that the compiled kernels hold no m0 reference other than these issues.
//  * vmcnt.  The load is inline asm so that the compiler's waitcnt pass does not know it: it adds no vmcnt(0) in
//    front of the LDS reads of the ring's other stages.  The caller waits for its own pieces explicitly (s_waitcnt
//    vmcnt(n), counting one per issue) before the barrier that publishes the stage.
// (rowgemm3.hip stages its panels with __builtin_amdgcn_global_load_lds instead: the compiler tracks that one and
// the kernel's barrier retires it.)
#pragma once
#include <stdint.h>

#include "common.h"

namespace mmpfn {

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// flat form: lane i's 16 B at its own address src
__device__ __forceinline__ void lds_dma16(const void* src, unsigned lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds) : "memory", "m0");
}
// saddr form: lane i's 16 B at sbase + voff, a scalar base per piece and one 32-bit offset VGPR for all of them (a
// 64-bit VGPR address per piece cost ~19 VGPRs at featrow.hip's register peak)
__device__ __forceinline__ void lds_dma16(uint32_t voff, const void* sbase, unsigned lds) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds)
               : "memory", "m0");
}
#pragma clang diagnostic pop

}  // namespace mmpfn
