// The LDS ring of the big-tile 16-bit GEMMs (gemm.hip gemm_glu_big_kernel / gemm_remap_big_kernel, modality.hip
// gemm_tile_kernel): 512-thread blocks, K in 32-wide slices, one slice of the block's A rows and W rows per stage.
//
// A stage is 512 unpadded 64-B rows (the A rows first, then the W rows: 256 + 256 or 320 + 192), 32 KB, with 16-B
// chunk c of row r at slot swz64(r, c) (conflict-free ds_read_b128 for the 16x16x32 operands).  It is filled by
// LDS-DMA (lds_dma.h), which writes lane-linear: a wave's piece j is the 1 KB at (wave * RING_DMA + j) * 1024 of the
// stage, so each lane fetches the chunk that belongs at its slot (ring_piece).  Every thread issues RING_DMA pieces
// per slice; "s slices may still be in flight" is therefore vmcnt(s * RING_DMA), and ring_wait holds the only
// ladder that spells it.  Each kernel keeps its own A / W addressing, main-loop schedule and epilogue
// (gemm_tile_kernel also its fragment read, ring_read written out: see the note there).
#pragma once
#include "common.h"
#include "lds_dma.h"

namespace mmpfn {

constexpr int RING_K = 32;                                  // K per slice
constexpr int RING_ROW = RING_K * 2;                        // 64-B LDS rows
constexpr int RING_ROWS = 512;                              // A rows + W rows of a stage
constexpr int RING_STAGE = RING_ROWS * RING_ROW;            // 32 KB
constexpr int RING_DMA = RING_ROWS * (RING_ROW / 16) / 512; // 16-B DMA pieces per thread and slice (4)

__device__ __forceinline__ int swz64(int r, int c) { return c ^ ((r >> 1) & 3); }

// this lane's share of its wave's piece j: stage row r and the global 16-B chunk c of that row
__device__ __forceinline__ void ring_piece(int wave, int lane, int j, int& r, int& c) {
  const int q = (wave * RING_DMA + j) * 64 + lane;
  r = q >> 2, c = swz64(r, q & 3);
}

// slice kt -> stage kt % NST; src[j]: the lane's address of piece j at slice 0
template <int NST, typename T>
__device__ __forceinline__ void ring_issue(const T* const (&src)[RING_DMA], int kt, unsigned lds0, int wave) {
  const unsigned base = lds0 + (kt % NST) * RING_STAGE + wave * RING_DMA * 1024;
#pragma unroll
  for (int j = 0; j < RING_DMA; ++j)
    lds_dma16(src[j] + kt * RING_K, __builtin_amdgcn_readfirstlane(base + j * 1024));
}

// this thread's pieces of every slice but the `ahead` issued last have landed; MAX: the caller's bound on `ahead`
// (a ring of NST stages keeps at most NST - 1 slices in flight: MAX <= 4 covers five stages)
template <int MAX>
__device__ __forceinline__ void ring_wait(int ahead) {
  static_assert(MAX >= 0 && MAX <= 4, "vmcnt ladder");
  if (MAX >= 4 && ahead >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * RING_DMA) : "memory");
  else if (MAX >= 3 && ahead == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * RING_DMA) : "memory");
  else if (MAX >= 2 && ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * RING_DMA) : "memory");
  else if (MAX >= 1 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RING_DMA) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// operand fragments of wave (wm, wn) of 2 x 4: MT 16-row A tiles from row wm * 16 MT, NT 16-row W tiles from W row
// wn * 16 NT (the W rows start A_ROWS into the stage); lane (fr, fg) holds row fr, K 8 fg .. 8 fg + 7 of each
template <int A_ROWS, typename X8, int MT, int NT>
__device__ __forceinline__ void ring_read(const unsigned char* stage, int wm, int wn, int fr, int fg, X8 (&af)[MT],
                                          X8 (&bw)[NT]) {
  static_assert(2 * 16 * MT == A_ROWS && A_ROWS + 4 * 16 * NT == RING_ROWS, "the eight waves cover the stage");
  const unsigned char* Ws = stage + A_ROWS * RING_ROW;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int rb = wn * (16 * NT) + i * 16 + fr;
    bw[i] = *(const X8*)(Ws + rb * RING_ROW + 16 * swz64(rb, fg));
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int ra = wm * (16 * MT) + i * 16 + fr;
    af[i] = *(const X8*)(stage + ra * RING_ROW + 16 * swz64(ra, fg));
  }
}

}  // namespace mmpfn
