// The render path's fused PE -> NeRF MLP forward (R4-R6; reference src/models.py:105-162, :14-47)
// on v_mfma_f32_16x16x32_f16: mlp16_kernel's split-f16 arithmetic ("f16x3", mlp16.hip) and weight
// stream (stream16.h, the same packed chunks), with 16 x 16 output tiles instead of 32 x 32.
//
// Why.  The MLP runs against the part's power limit, not its issue rate: mlp16_kernel
// holds 1.78-1.85 GHz.  The 16x16x32 instruction does the same FLOP in the same cycles per SIMD, but
// under that limit the chip holds it at a higher clock (MI355X_MICROARCH "DVFS give-back" 7; on the
// trunk's half-step with its side work, scripts/microbench/mfma_shape_side.hip measured +2-5 %,
// profiles/r02_mfma_shape_side.log).  This kernel serves the render calls (nerf_render_rays,
// nerf_mlp_forward); the training forward with saves and the data-gradient kernels keep the 32 x 32
// shape (their mask and save layouts follow it).
//
// Layout.  A wave still owns 32 samples and runs the whole network for them, as two sample tiles
// st = 0, 1 (samples 16 st + (lane & 15)).  Lane l sits in lane group g = l >> 4; per MFMA it supplies
// row / column l & 15 and the 8 k values 8g .. 8g+7 of a 32-deep k-step.
//  * Weights (A): a k-step of 32 is one stream chunk's two 16-deep k-steps.  mlp16's 1 KiB piece
//    (tile T of 32 rows, old k-step kk, hi or lo part) holds W[32T + (p & 31)][k-group p >> 5] in
//    lane p; the 16 x 32 fragment of row half r reads, in lane l, piece kk = g >> 1's lane
//    R_r(l & 15) + 32 (g & 1), with R_r(i) = (i & 7) + 8r + 16 (i >> 3): a per-lane LDS address, the
//    packed stream unchanged.
//  * Outputs: the 16 x 16 tile (T, r, st) holds neuron 32T + R_r(4g + e) of sample 16 st + (l & 15)
//    in lane l, register e: neuron 32T + 8r + 4 (g & 1) + 16 (g >> 1) + e.
//  * Activations (B): the next layer's 32-deep k-step T reads in lane l (sample tile st) elements
//    4r + e = tile (T, r, st)'s register e as it stands: exactly the input order mlp16's packed k
//    order gives the 16-deep k-steps 2T, 2T+1 (layout.h s16_source_col), so the operands are built
//    in place, as in mlp16.
//  * PE: lane group g = 2s + h supplies PE slot 8 (2t + s) + j of k-step t (sin for h = 0, cos for
//    h = 1, layout.h pe_feature): 16 of the sample's slots per lane, for each of its 2 samples.
// Each lane holds two samples: scales, maxima, the density dot product and the colour head are kept
// per sample tile, and a sample's maximum / sums run over its 4 lane groups (xor 16, xor 32).
//
// Weight stream (per 16 KiB chunk = one 32-deep k-step of a 4-tile group): 4 tile segments of 12
// MFMAs (2 row halves x 2 sample tiles x 3 products).  A tile's fragments (4: row half x hi/lo) are
// read into its own 16 registers one chunk ahead: tile 3's at the chunk's segment 0, tiles 0-2 of the
// next chunk in segments 1-3, each right after the registers' last MFMAs; the next chunk is published
// (counted vmcnt + barrier, as stream16.h) after segment 0 and the chunk three ahead is DMA'd in
// segments 1-3: wave w moves the chunk's four consecutive 1 KiB pieces 4w .. 4w+3 from one address
// pair and one M0 write, the pieces told apart by the instruction's immediate offset (sdma_piece).
// The previous layer's epilogue (the side work) runs in the MFMA shadow.  In the plain trunk (layers
// 1-3, 5-6 and layer 7's group A) it runs as half-quarters (two values of a 16 x 16 tile of one
// sample tile), one per segment, placed by hand at no more than two VALU instructions per MFMA gap
// and with no packed-f32 instruction (ssegment_h, shalf).  Layer 0, the skip layer, layer 7's group
// B and the colour layer, whose segments also carry PE work, keep a quarter (4 values) per segment
// on mlp16's group schedule (ssegment, squarter).
//
// Block loop.  The grid is one workgroup per CU; workgroup b runs the 128-sample blocks b, b + grid,
// ...  Biases, constants and the rgb head are staged in LDS once per workgroup.  The weight ring does
// not drain between blocks: the colour layer's chunk-steps fetch the wrapped stream's chunks 0-2 and
// read chunk 0's first fragments, so a block starts at layer 0's first MFMA.  The next block's inputs
// are loaded during layer 7, and its positional encoding and layer-0 operands are computed as side
// work in the 32 segments of layer 7's group B and of the colour layer that carry no quarter.  Per
// sample the arithmetic is the one-block kernel's, operation for operation (DESIGN §4 has the stamps
// and the same-box A/B of each step).  The loop's body holds no division (a sample's ray is a
// multiply-high by the launcher's reciprocal of N, sample_index.h; the scales' reciprocals are exponent
// arithmetic) and no branch ahead of the heads: a branch ends the basic block, and the compiler sinks
// work out of the MFMA shadow into the block behind it.
#include <atomic>
#include "common.h"
#include "pe_sin.h"
#include "stream16.h"

namespace nerf {

// Diagnostic build (scripts/microbench/mlp16s_stamps.hip, never the library): per-wave s_memtime stamps,
// kept in LDS words of the wave's own (LDS writes leave the stream's counted vmcnt alone) and copied to
// a buffer of their own after the wave's last store.  Stamps: 0 entry | 1 first MFMA | 2 + L end of
// trunk layer L (0..7) | 10 end of the colour layer | 11 last store; 12, 13: s_memrealtime at 0 and 11.
#ifdef NERF_MLP16S_STAMPS
__device__ unsigned long long nerf16s_stamps[65536][16];
constexpr int kSStampFloats = kW16Waves * 32;
constexpr int kSStampIter = 8;   // the block (of the workgroup's) that is stamped
#define STAMP16S_ASM(i, insn)                                                               \
  do {                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    unsigned long long t_;                                                                  \
    asm volatile(insn " %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                 \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    if (lane == 0 && stamp_on) reinterpret_cast<unsigned long long*>(lds + kSLdsFloats)[wave * 16 + (i)] = t_; \
  } while (0)
#define STAMP16S(i) STAMP16S_ASM(i, "s_memtime")
#define STAMP16S_REAL(i) STAMP16S_ASM(i, "s_memrealtime")
#else
constexpr int kSStampFloats = 0;
#define STAMP16S(i) do {} while (0)
#define STAMP16S_REAL(i) do {} while (0)
#endif

__device__ __forceinline__ f32x4 mfma16s(h16x8 a, h16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// LDS: [ring 4 x 16 KiB][PE: 4 waves x 2 samples x 16 slots x 64 lanes][biases | density_head w, b]
// [layer constants][rgb_linear][per-wave ray features] (mlp16.hip's layout)
constexpr int kSLdsPe = 4 * kChunkFloats;
constexpr int kSLdsBias = kSLdsPe + kW16Waves * kPeSteps * 64;
constexpr int kSLdsSigmaW = kSLdsBias + 8 * kHidden;
constexpr int kSLdsVecFloats = 8 * kHidden + kHidden + 4;
constexpr int kSLdsConsts = kSLdsBias + kSLdsVecFloats;
constexpr int kSLdsRgb = kSLdsConsts + kS16Consts;
constexpr int kSLdsRgbFloats = 3 * kDirHidden + 4;
constexpr int kSLdsFeat = kSLdsRgb + kSLdsRgbFloats;
constexpr int kSLdsFloats = kSLdsFeat + kW16Waves * kRayFeat;
static_assert(kSLdsRgb % 4 == 0 && kSLdsFeat % 4 == 0, "LDS vector layout");
static_assert((kS16Chunks & (kS16Chunks - 1)) == 0 && kS16Chunks % 4 == 0, "the stream wraps onto the same ring slots");

typedef h16x8 STile[2][2];   // a tile's fragments: [row half][hi, lo]
typedef f32x4 SAcc[8][2][2]; // [tile][row half][sample tile]

// Tile TI's 4 fragments of the chunk in `slot`: off[r] = the lane's float offset of row half r
template <int TI>
__device__ __forceinline__ void sread_tile(const float* slot, const uint32_t (&off)[2], STile& a) {
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int part = 0; part < 2; ++part)
      a[r][part] = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(slot + off[r] + TI * 512 + part * 256));
}

// Fragment K (row half K >> 1, hi / lo K & 1) of tile TI: sread_tile's reads one at a time
template <int TI, int K>
__device__ __forceinline__ void sread_frag(const float* slot, const uint32_t (&off)[2], STile& a) {
  constexpr int r = K >> 1, part = K & 1;
  a[r][part] = __builtin_bit_cast(h16x8, *reinterpret_cast<const f32x4*>(slot + off[r] + TI * 512 + part * 256));
}

// ---- the render kernel's weight DMA --------------------------------------------------------
// Wave w moves the four consecutive 1 KiB pieces 4w .. 4w+3 of a chunk (stream16.h's chunk_dma_piece
// gives it w, w+4, w+8, w+12: an M0 write, its wait state and a 64-bit address per piece, 16 scalar
// instructions per chunk-step on the issue port of the SIMD's only wave).  The instruction's
// immediate offset moves the global address and the LDS destination together (LDS address = M0 +
// offset + 16 lane; scripts/microbench/lds_dma_offset.hip checks it on the device), so piece I is
// offset:1024 I from one SGPR pair and one M0 value per chunk: piece 0 writes M0, pieces 1-3 read
// what it left.  That holds while nothing writes M0 between a chunk's pieces: the feature-row DMA
// restores it, and scripts/check_isa.py checks the built kernel (its "held M0" rule).
// lds_base: the ring's LDS byte address + kSDmaWave * wave; voff = 16 lane + kSDmaWave * wave.
#ifdef NERF16S_PIECE_DMA   // A/B build: stream16.h's assignment
constexpr uint32_t kSDmaWave = 1024;
template <int SLOT, int I>
__device__ __forceinline__ void sdma_piece(const float* __restrict__ stream, int c, uint32_t lds_base, uint32_t voff) {
  chunk_dma_piece<SLOT, I>(stream, c, lds_base, voff);
}
#else
constexpr uint32_t kSDmaWave = 4096;
template <int SLOT, int I>
__device__ __forceinline__ void sdma_piece(const float* __restrict__ stream, int c, uint32_t lds_base, uint32_t voff) {
  const char* src = reinterpret_cast<const char*>(stream) + (size_t)c * (kChunkFloats * 4);
  if constexpr (I == 0)
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(src), "s"(lds_base + SLOT * (kChunkFloats * 4))
        : "memory", "m0");
  else
    asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(voff), "s"(src), "n"(I * 1024) : "memory");
}
#endif
template <int SLOT>
__device__ __forceinline__ void sdma_chunk(const float* __restrict__ stream, int c, uint32_t lds_base, uint32_t voff) {
  sdma_piece<SLOT, 0>(stream, c, lds_base, voff);
  sdma_piece<SLOT, 1>(stream, c, lds_base, voff);
  sdma_piece<SLOT, 2>(stream, c, lds_base, voff);
  sdma_piece<SLOT, 3>(stream, c, lds_base, voff);
}

// Tile TI's 12 MFMAs: per (row half, sample tile) lo(W)hi(a), hi(W)lo(a), hi(W)hi(a) chained.
// hook(j) after chain j (the DMA pieces).
template <int G, int TI, bool FIRST, typename Hook>
__device__ __forceinline__ void smfma_tile(const STile& a, const Operand& b0, const Operand& b1, SAcc& acc,
                                           Hook&& hook) {
  static_for<4>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value, r = j >> 1, st = j & 1;
    const Operand& b = st ? b1 : b0;
    f32x4 c;
    if constexpr (FIRST) c = mfma16s(a[r][1], b.hi, f32x4{});
    else c = mfma16s(a[r][1], b.hi, acc[4 * G + TI][r][st]);
    c = mfma16s(a[r][0], b.lo, c);
    acc[4 * G + TI][r][st] = mfma16s(a[r][0], b.hi, c);
    hook(jc);
  });
}

// One tile segment: side work phase 0 (its LDS reads first), the fragment reads (NRD tiles' worth,
// `reads`), tile TI's MFMAs (+ hook), side phase 1, interleaved: per MFMA gap one MFMA, one DS read
// (gaps 1..4 per tile read), VPG VALU from gap kSValuGap0 on.  The side's VALU waits for its LDS reads
// (biases, density weights), issued at the segment's start; a 16x16x32 MFMA issues in half the cycles
// of a 32x32x16 one, so mlp16's gap 1 left them ~2 MFMAs of cover and the in-order wave stalled
// there with the MFMA pipe drained.  From gap 5 (7 gaps of VALU): +2.2-2.9 % frame rate, same box
// (gap 3 +1.9 %, 4 and 6 within 0.2 % of 5, 7 the same, 9 +1.2-2.5 %; profiles/r06/ab_render_vgap*.log).
constexpr int kSValuGap0 = 5;
template <int G, int TI, bool FIRST, int NRD, int VPG, typename Reads, typename Side, typename Hook>
__device__ __forceinline__ void ssegment(const STile& a, const Operand& b0, const Operand& b1, SAcc& acc, Reads&& reads,
                                         Side&& side, Hook&& hook) {
  side(std::integral_constant<int, 0>{});
  __builtin_amdgcn_sched_barrier(0);
  reads();
  smfma_tile<G, TI, FIRST>(a, b0, b1, acc, hook);
  side(std::integral_constant<int, 1>{});
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // 1 MFMA
    if (i >= 1 && i <= 4 * NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
    if (VPG > 0 && i >= kSValuGap0) __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);   // VALU
  }
  __builtin_amdgcn_sched_barrier(0);
}

// The plain trunk's tile segment (layers 1-3, 5-6, layer 7's group A), placed by hand: every MFMA gap
// is fenced, so what a gap holds is what is written here.  The side work comes as half-quarters (two
// values of a quarter, 10 VALU in 6 units of at most two: shalf below), one per segment, at most two
// VALU per gap, in gaps that carry neither a fragment read (1-4) nor a DMA piece (2, segment 1's 8):
// an MFMA holds the issue port for 8 of its 16 cycles and a VALU instruction for 4, so a third
// instruction in a gap lengthens it.  The quarter schedule above put six per gap into four gaps
// of every other segment (its 40-VALU budget against the ~20 the quarter has).  A group has 32
// halves and 28 segments that may carry one; four segments carry two, one gap apart (and then in
// the gap of a DMA piece too).
// side(slot, unit): unit -1 the half's LDS read, 0..5 its VALU units; slot 0, 1 the segment's halves.
// the unit (or -2) in `gap`: a lone half in gaps 5, 6, 7, 9, 10, 11; a segment's two halves in gaps
// 5-10 and 6-11, a unit apart, so that no gap holds the same instruction of both
__device__ __forceinline__ constexpr int shalf_unit_at(int gap, int slot, bool two) {
  if (two) return gap >= 5 + slot && gap <= 10 + slot ? gap - 5 - slot : -2;
  return slot ? -2 : (gap >= 5 && gap <= 7 ? gap - 5 : (gap >= 9 && gap <= 11 ? gap - 6 : -2));
}
template <int G, int TI, bool FIRST, int NRD, bool TWO, typename Frag, typename Side, typename Hook>
__device__ __forceinline__ void ssegment_h(const STile& a, const Operand& b0, const Operand& b1, SAcc& acc, Frag&& frag,
                                           Side&& side, Hook&& hook) {
  using Slot0 = std::integral_constant<int, 0>;
  using Slot1 = std::integral_constant<int, 1>;
  side(Slot0{}, std::integral_constant<int, -1>{});
  side(Slot1{}, std::integral_constant<int, -1>{});
  __builtin_amdgcn_sched_barrier(0);
  static_for<12>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value, j = i / 3, k = i % 3, r = j >> 1, st = j & 1;
    const Operand& b = st ? b1 : b0;
    f32x4& c = acc[4 * G + TI][r][st];
    if constexpr (k == 0) c = FIRST ? mfma16s(a[r][1], b.hi, f32x4{}) : mfma16s(a[r][1], b.hi, c);
    if constexpr (k == 1) c = mfma16s(a[r][0], b.lo, c);
    if constexpr (k == 2) {
      c = mfma16s(a[r][0], b.hi, c);
      hook(std::integral_constant<int, j>{});
    }
    if constexpr (i >= 1 && i <= 4 * NRD) frag(std::integral_constant<int, i - 1>{});
    side(Slot0{}, std::integral_constant<int, shalf_unit_at(i, 0, TWO)>{});
    side(Slot1{}, std::integral_constant<int, shalf_unit_at(i, 1, TWO)>{});
    __builtin_amdgcn_sched_barrier(0);
  });
}

// Side-work schedules, by (chunk i of the group, segment): which quarter (or PE operand) runs there.
enum SSide { kSNone, kSPrev, kSCur, kSL0, kSSkipPrev, kSSkipCur, kSPrevPe, kSCurPe, kSPrevH, kSCurH };
// The skip layer's PE operands (k-steps 8, 9; two sample tiles each) are split from the wave's LDS
// copy just before each group reads them: k-step 8's in chunk 7 (segments 0, 2), 9's in chunk 8
// (segments 0, 2), so they hold registers only while read (the rest of the layer needs all of in[]).
__device__ __forceinline__ constexpr int spe_at(int i, int seg) {
  return (i == 7 || i == 8) && (seg == 0 || seg == 2) ? 2 * (i - 7) + seg / 2 : -1;   // operand 2 t + st
}
// group A's side (the previous layer's tiles 4-7, quarters 0..15): 3, 3, 2, 2, 2, 2, 2 per chunk
// (chunks 0..6; tile 4+j's quarters are done before chunk 4+j reads them).  Segments: three
// quarters in segments 1-3, two in 1 and 3.
__device__ __forceinline__ constexpr int sq_prev(int i, int seg) {
  constexpr int base[7] = {0, 3, 6, 8, 10, 12, 14};
  if (i >= 7) return -1;
  const int n = i < 2 ? 3 : 2;
  if (n == 3) return seg >= 1 ? base[i] + seg - 1 : -1;
  return seg == 1 ? base[i] : (seg == 3 ? base[i] + 1 : -1);
}
// group B's side (this layer's tiles 0-3, quarters 0..15): 0, 2, 2, 2, 2, 3, 3, 2 per chunk (tile T's
// quarters only after chunk T has read its operands)
__device__ __forceinline__ constexpr int sq_cur(int i, int seg) {
  constexpr int base[8] = {0, 0, 2, 4, 6, 8, 11, 14};
  constexpr int cnt[8] = {0, 2, 2, 2, 2, 3, 3, 2};
  if (i >= 8 || cnt[i] == 0) return -1;
  if (cnt[i] == 3) return seg >= 1 ? base[i] + seg - 1 : -1;
  return seg == 1 ? base[i] : (seg == 3 ? base[i] + 1 : -1);
}
// The same two sides in half-quarters (kSPrevH, kSCurH; half h = quarter h >> 1's values 2 (h & 1),
// + 1), under the same two constraints.  Group A: two per segment in chunk 0, one in every segment of
// chunks 1-6.  Group B: one in every segment of chunks 1-6, two per segment in chunk 7.
__device__ __forceinline__ constexpr int sh_prev(int i, int seg, int slot) {
  if (i == 0) return 2 * seg + slot;
  return i >= 7 || slot ? -1 : 8 + 4 * (i - 1) + seg;
}
__device__ __forceinline__ constexpr int sh_cur(int i, int seg, int slot) {
  if (i == 7) return 24 + 2 * seg + slot;
  return i == 0 || i >= 8 || slot ? -1 : 4 * (i - 1) + seg;
}
__device__ __forceinline__ constexpr bool sh_schedules_hold() {
  int np = 0, nc = 0;
  for (int i = 0; i < 8; ++i)
    for (int seg = 0; seg < 4; ++seg)
      for (int slot = 0; slot < 2; ++slot) {
        const int hp = sh_prev(i, seg, slot), hc = sh_cur(i, seg, slot);
        if (hp >= 0 && (hp != np++ || i >= 4 + hp / 8)) return false;   // tile 4+j converted before chunk 4+j
        if (hc >= 0 && (hc != nc++ || i <= hc / 8)) return false;       // tile T only after chunk T
      }
  return np == 32 && nc == 32;
}
static_assert(sh_schedules_hold(), "half-quarter schedules: each half once, in order, inside its window");
// The next block's positional encoding (32 values per lane) runs one value per segment in the 32
// segments of layer 7's group B and of the colour layer (8 chunks each) that carry no quarter: value
// 0..15 in group B's free segments in order, 16..31 in the colour layer's.
template <bool CUR>
__device__ __forceinline__ constexpr int spe_next(int i, int seg) {
  if (i >= 8 || (CUR ? sq_cur(i, seg) : sq_prev(i, seg)) >= 0) return -1;
  int n = 0;
  for (int k = 0; k < 4 * i + seg; ++k) n += (CUR ? sq_cur(k / 4, k % 4) : sq_prev(k / 4, k % 4)) < 0;
  return n + (CUR ? 0 : 16);
}
static_assert(spe_next<true>(7, 2) == 15 && spe_next<false>(7, 3) == 31, "32 free segments");
template <int KIND>
__device__ __forceinline__ constexpr int side_count(int i, int seg) {
  if constexpr (KIND == kSPrevPe || KIND == kSCurPe) return 1;
  if constexpr (KIND == kSPrev) return sq_prev(i, seg) >= 0;
  if constexpr (KIND == kSSkipPrev) return (sq_prev(i, seg) >= 0) + (spe_at(i, seg) >= 0);
  if constexpr (KIND == kSCur) return sq_cur(i, seg) >= 0;
  if constexpr (KIND == kSSkipCur) return (sq_cur(i, seg) >= 0) + (spe_at(i, seg) >= 0);
  if constexpr (KIND == kSL0) return 2;
  return 0;
}
template <int KIND>
__device__ __forceinline__ constexpr int svpg(int i, int seg) {
  const int n = side_count<KIND>(i, seg);
  return n == 0 ? 0 : (n * 40 + 11 - kSValuGap0) / (12 - kSValuGap0);   // ~40 VALU per quarter
}

// Segment TI of chunk I under side schedule KIND: the hand-placed segment for the half-quarter
// schedules, the group-scheduled one for the rest.  frag(K) reads fragment K of the segment's tile.
template <int G, int TI, bool FIRST, int NRD, int KIND, int I, typename Frag, typename Side, typename Hook>
__device__ __forceinline__ void sseg(const STile& a, const Operand& b0, const Operand& b1, SAcc& acc, Frag&& frag,
                                     Side&& side, Hook&& hook) {
  using IC = std::integral_constant<int, I>;
  using SC = std::integral_constant<int, TI>;
  if constexpr (KIND == kSPrevH || KIND == kSCurH) {
    constexpr bool two = (KIND == kSPrevH ? sh_prev(I, TI, 1) : sh_cur(I, TI, 1)) >= 0;
    ssegment_h<G, TI, FIRST, NRD, two>(a, b0, b1, acc, frag, [&](auto slot, auto unit) __attribute__((always_inline)) {
      side(IC{}, SC{}, slot, unit);
    }, hook);
  } else {
    ssegment<G, TI, FIRST, NRD, svpg<KIND>(I, TI)>(a, b0, b1, acc, [&]() __attribute__((always_inline)) {
      static_for<4>(frag);
    }, [&](auto ph) __attribute__((always_inline)) { side(IC{}, SC{}, ph); }, hook);
  }
}

// One chunk-step: chunk c (global index, ring slot SLOT) = k-step i of group G; b0 / b1 its sample
// tiles' operands.  On entry chunk c is published and tiles 0-2 of its fragments are in a[0..2].
// TAIL = chunks left after c (capped at 3).
// WRAP (the colour layer in the block loop): the chunk three ahead is taken modulo the 128-chunk
// stream, a multiple of the 4-slot ring, so the next block's chunks keep their slots.
// pub(I) runs right behind the publish: the only pieces in flight there are chunk c+2's, a chunk-step
// old, so a compiler-counted wait for loads of the kernel's own costs next to nothing there.
struct SNoPub {
  template <typename I>
  __device__ __forceinline__ void operator()(I) const {}
};
template <int G, int SLOT, bool FIRST, int TAIL, int KIND, int I, bool WRAP, typename Side, typename Pub>
__device__ __forceinline__ void schunk(const float* __restrict__ stream, int c, float* lds, uint32_t lds_dma,
                                       uint32_t voff, const uint32_t (&off)[2], STile (&a)[4], const Operand& b0,
                                       const Operand& b1, SAcc& acc, Side&& side, Pub&& pub) {
  const float* cur = lds + SLOT * kChunkFloats;
  const float* nxt = lds + ((SLOT + 1) & 3) * kChunkFloats;
  auto none = [](auto) {};
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  using S3 = std::integral_constant<int, 3>;
  // segment 0: this chunk's tile 3 fragments (their registers' last MFMAs were the previous chunk's)
  sseg<G, 0, FIRST, 1, KIND, I>(a[0], b0, b1, acc, [&](auto kc) __attribute__((always_inline)) {
    sread_frag<3, decltype(kc)::value>(cur, off, a[3]);
  }, side, none);
  // publish chunk c+1: own DMA pieces landed (younger: chunk c+2's 4), barrier
  if constexpr (TAIL >= 1) {
    wait_vmcnt<TAIL >= 2 ? 4 : 0>();
    __builtin_amdgcn_s_barrier();
  }
  pub(std::integral_constant<int, I>{});
  // DMA of chunk c+3 into the slot chunk c-1 used (every wave's reads of it fed MFMAs issued before
  // the barrier): pieces 0, 1 in segment 1, 2 and 3 in segments 2, 3, after a chain's MFMAs
  auto dma = [&](auto pc) __attribute__((always_inline)) {
    if constexpr (TAIL >= 3)
      sdma_piece<(SLOT + 3) & 3, decltype(pc)::value>(stream, WRAP ? (c + 3) & (kS16Chunks - 1) : c + 3, lds_dma, voff);
  };
  sseg<G, 1, FIRST, (TAIL >= 1), KIND, I>(a[1], b0, b1, acc, [&](auto kc) __attribute__((always_inline)) {
    if constexpr (TAIL >= 1) sread_frag<0, decltype(kc)::value>(nxt, off, a[0]);
  }, side, [&](auto jc) __attribute__((always_inline)) {
    if constexpr (decltype(jc)::value == 0) dma(S0{});
    if constexpr (decltype(jc)::value == 2) dma(S1{});
  });
  sseg<G, 2, FIRST, (TAIL >= 1), KIND, I>(a[2], b0, b1, acc, [&](auto kc) __attribute__((always_inline)) {
    if constexpr (TAIL >= 1) sread_frag<1, decltype(kc)::value>(nxt, off, a[1]);
  }, side, [&](auto jc) __attribute__((always_inline)) {
    if constexpr (decltype(jc)::value == 0) dma(S2{});
  });
  sseg<G, 3, FIRST, (TAIL >= 1), KIND, I>(a[3], b0, b1, acc, [&](auto kc) __attribute__((always_inline)) {
    if constexpr (TAIL >= 1) sread_frag<2, decltype(kc)::value>(nxt, off, a[2]);
  }, side, [&](auto jc) __attribute__((always_inline)) {
    if constexpr (decltype(jc)::value == 0) dma(S3{});
  });
}

// A group of NSTEP chunk-steps from global chunk c0 (ring slot SLOT0); operand(i, st) gives k-step
// i's B operand of sample tile st.  TAIL_END = chunks after this group (capped at 3).
template <int G, int NSTEP, int SLOT0, int TAIL_END, int KIND, bool WRAP = false, typename Opnd, typename Side,
          typename Pub = SNoPub>
__device__ __forceinline__ void sgroup(const float* __restrict__ stream, int c0, float* lds, uint32_t lds_dma,
                                       uint32_t voff, const uint32_t (&off)[2], STile (&a)[4], SAcc& acc,
                                       Opnd&& operand, Side&& side, Pub&& pub = Pub{}) {
  static_for<NSTEP>([&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    constexpr int left = NSTEP - 1 - i + TAIL_END;
    schunk<G, (SLOT0 + i) & 3, i == 0, (left < 3 ? left : 3), KIND, i, WRAP>(
        stream, c0 + i, lds, lds_dma, voff, off, a, operand(ic, std::integral_constant<int, 0>{}),
        operand(ic, std::integral_constant<int, 1>{}), acc, side, pub);
  });
}

// A layer's tiles 4-7 stay in their accumulator registers across the layer's edge (the layer loop's
// back edge, a peeled layer's entry): opaque there in the `a` class, each value is copied out where the
// next layer's side work converts it.  Left to itself the compiler copies all 64 values to vector
// registers at the edge, in one burst with the matrix pipe empty, and keeps them there.
__device__ __forceinline__ void sacc_hold(SAcc& acc) {
#ifndef NERF16S_EDGE_BURST   // (A/B build: the compiler's copies)
#pragma unroll
  for (int T = 4; T < 8; ++T)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int st = 0; st < 2; ++st) asm volatile("" : "+a"(acc[T][r][st]));
#endif
}

// The sample's value over its 4 lane groups.  The exchange is gfx950's row and half swaps of two
// copies of the value (v_permlane16_swap: the first copy's odd 16-lane rows against the second's even
// rows; v_permlane32_swap: the first's upper half against the second's lower half), after which the
// two copies hold both partners in every lane: two VALU instructions where __shfl_xor takes a
// ds_bpermute round trip.  smax4 sits between a layer's two groups with the matrix pipe empty, four
// dependent round trips per layer.  max and + commute, so each lane combines the same two values as
// with __shfl_xor(., 16) and __shfl_xor(., 32): the same bits.
typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
template <typename F>
__device__ __forceinline__ float sover4(float v, F&& f) {
#ifdef NERF16S_SHFL_REDUCE   // (A/B build: the shuffles)
  v = f(v, __shfl_xor(v, 16));
  return f(v, __shfl_xor(v, 32));
#else
  const u32x2s a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = f(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const u32x2s b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return f(__uint_as_float(b[0]), __uint_as_float(b[1]));
#endif
}
__device__ __forceinline__ float smax4(float m) {
  return sover4(m, [](float x, float y) { return fmaxf(x, y); });
}
__device__ __forceinline__ float ssum4(float v) {
  return sover4(v, [](float x, float y) { return x + y; });
}

struct SQuarter {
  f32x4 b, w;
};

// Quarter QG (0..15) of the 4-tile group from tile T0: tile T = T0 + QG / 4, row half r and sample
// tile st = (QG % 4) >> 1, QG % 2 -> elements 4r .. 4r+3 of operand in[2T + st].  Phase 0 reads the
// bias (and density weights) from LDS, phase 1 converts: y = ReLU(acc inv + b), max, (SIGMA) density
// dot, split at the sample's scale.
template <int PH, int T0, int QG, bool SIGMA>
__device__ __forceinline__ void squarter(const SAcc& acc, const float (&inv)[2], const float* bias, const float* ws,
                                         int nlane, const float (&sc)[2], Operand (&in)[16], float (&m)[2],
                                         float (&part)[2], SQuarter& qv) {
  constexpr int T = T0 + QG / 4, r = (QG % 4) >> 1, st = QG & 1;
  const int n0 = 32 * T + 8 * r + nlane;
  if constexpr (PH == 0) {
    qv.b = *reinterpret_cast<const f32x4*>(bias + n0);
    if constexpr (SIGMA) qv.w = *reinterpret_cast<const f32x4*>(ws + n0);
  } else {
    float xs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float y = fmaxf(fmaf(acc[T][r][st][e], inv[st], qv.b[e]), 0.0f);
      m[st] = fmaxf(m[st], y);
      if constexpr (SIGMA) part[st] = fmaf(qv.w[e], y, part[st]);
      xs[e] = y * sc[st];
    }
    Operand& op = in[2 * T + st];
    typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const h16x2 hi2 = {(_Float16)xs[2 * p], (_Float16)xs[2 * p + 1]};
      const h16x2 lo2 = __builtin_bit_cast(h16x2, split_lo_pair(__builtin_bit_cast(uint32_t, hi2), xs[2 * p], xs[2 * p + 1]));
      const int j = 4 * r + 2 * p;
      op.hi[j] = hi2[0];
      op.hi[j + 1] = hi2[1];
      op.lo[j] = lo2[0];
      op.lo[j + 1] = lo2[1];
    }
  }
}

// `v` made to depend on `after` (no instruction): two values the compiler sees as dependent are not
// paired into one packed-f32 instruction.  Beside MFMAs a v_pk_fma_f32 or v_pk_mul_f32 costs more
// than the two instructions it replaces (MI355X: +22 cycles per v_pk_fma_f32).  `v` is first read
// an MFMA gap later: the compiler puts an s_nop between an asm statement and a reader of its output.
__device__ __forceinline__ void sunpaired(float& v, float after) {
#ifndef NERF16S_PACKED_SIDE   // (A/B build: the compiler's pairing)
  asm("" : "+v"(v) : "v"(after));
#endif
}

typedef float f32x2s __attribute__((ext_vector_type(2)));
struct SHalf {
  f32x2s b;
  float y[2], xs[2];
};

// Half H (0..31) of the 4-tile group from tile T0: values 2p, 2p + 1 (p = H & 1) of quarter H >> 1,
// squarter's arithmetic for them operation for operation (no density dot: the trunk's sides have
// none), as units of at most two VALU instructions, one unit per MFMA gap (ssegment_h).  The second
// value runs a unit behind the first, so that a gap's two instructions are of different kinds:
//   -1 the bias read | 0 y0 = acc inv + b | 1 y1, ReLU y0 | 2 ReLU y1, x0 = y0 sc | 3 x1, maximum |
//   4 the f16 hi pair | 5 the lo pair
template <int U, int T0, int H>
__device__ __forceinline__ void shalf(const SAcc& acc, const float (&inv)[2], const float* bias, int nlane,
                                      const float (&sc)[2], Operand (&in)[16], float (&m)[2], SHalf& hv) {
  constexpr int QG = H >> 1, p = H & 1, T = T0 + QG / 4, r = (QG % 4) >> 1, st = QG & 1, j = 4 * r + 2 * p;
  typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
  Operand& op = in[2 * T + st];
  if constexpr (U == -1) hv.b = *reinterpret_cast<const f32x2s*>(bias + 32 * T + 8 * r + nlane + 2 * p);
  if constexpr (U == 0) {
    hv.y[0] = fmaf(acc[T][r][st][2 * p], inv[st], hv.b[0]);
    float b1 = hv.b[1];
    sunpaired(b1, hv.y[0]);
    hv.b[1] = b1;
  }
  if constexpr (U == 1) {
    hv.y[1] = fmaf(acc[T][r][st][2 * p + 1], inv[st], hv.b[1]);
    hv.y[0] = fmaxf(hv.y[0], 0.0f);
  }
  if constexpr (U == 2) {
    hv.y[1] = fmaxf(hv.y[1], 0.0f);
    hv.xs[0] = hv.y[0] * sc[st];
    sunpaired(hv.y[1], hv.xs[0]);
  }
  if constexpr (U == 3) {
    hv.xs[1] = hv.y[1] * sc[st];
    m[st] = fmaxf(fmaxf(m[st], hv.y[0]), hv.y[1]);
  }
  if constexpr (U == 4) {
    const h16x2 hi2 = {(_Float16)hv.xs[0], (_Float16)hv.xs[1]};
    op.hi[j] = hi2[0];
    op.hi[j + 1] = hi2[1];
  }
  if constexpr (U == 5) {
    const h16x2 hi2 = {op.hi[j], op.hi[j + 1]};
    const h16x2 lo2 = __builtin_bit_cast(h16x2, split_lo_pair(__builtin_bit_cast(uint32_t, hi2), hv.xs[0], hv.xs[1]));
    op.lo[j] = lo2[0];
    op.lo[j + 1] = lo2[1];
  }
}

// A segment's second half runs a unit behind its first (unit U of the second just done, U + 1 of the
// first before it): the second's scale products are kept from pairing with the first's.
template <int U>
__device__ __forceinline__ void shalf_follow(const SHalf& first, SHalf& second) {
  if constexpr (U == 1) sunpaired(second.y[0], first.xs[0]);
  if constexpr (U == 2) sunpaired(second.y[1], first.xs[1]);
}

// PE operand of k-step t, sample tile st, split at sc[st] from this wave's LDS copy: phase 0 reads the
// 8 values into v, phase 1 splits.
template <int PH, int t, int st>
__device__ __forceinline__ void spe_operand(const float* pe_mine, const float (&sc)[2], Operand& op, float (&v)[8],
                                            int lane) {
  if constexpr (PH == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = pe_mine[((st * 2 + t) * 8 + j) * 64 + lane];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) split_into(v[j] * sc[st], op, j);
  }
}

// The kernel, twice (mlp16s_body.h): mlp16s_kernel over the samples 0 .. M-1 of a launch, and
// mlp16s_live_kernel over the samples a device-side live list names (occupancy-grid sample skipping,
// occupancy.hip).  The second differs in where a block's sample indices come from, and reads its
// sample count on the device; the arithmetic per sample is the same text.
#define MLP16S_GATHER 0
#include "mlp16s_body.h"
#undef MLP16S_GATHER
#define MLP16S_GATHER 1
#include "mlp16s_body.h"
#undef MLP16S_GATHER

// Workgroups of the persistent grid: one per CU of the current device (the kernel's registers and its
// 111 KiB of LDS leave room for one workgroup per CU).  Read once per device.
static int device_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  int n = cached[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
    cached[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int launch_mlp16s(const float* packed, const float* o, const float* d, const float* z, int64_t R, int N,
                  const float* feat, float* rgb, float* sigma, const int* out_slot, int out_T, hipStream_t s) {
  const int64_t M = R * (int64_t)N;
  if (M == 0) return NERF_OK;
  constexpr int per_block = 32 * kW16Waves;
  const int64_t blocks = (M + per_block - 1) / per_block;
  const int cus = device_cus();
  if (cus <= 0) return set_error(NERF_ERR_HIP, "mlp16s_kernel: cannot read the device's CU count");
  const RayDiv nd = ray_div_of(N);   // sample -> ray without a division in the kernel
  hipLaunchKernelGGL(mlp16s_kernel, dim3((unsigned)(blocks < cus ? blocks : cus)), dim3(64 * kW16Waves), 0, s, packed, o, d, z, M, N, feat,
                     rgb, sigma, out_slot, out_T, nd.mul, nd.shift);
  return check_launch("mlp16s_kernel");
}

// The gathered launch (nerf_mlp_forward_live, nerf_render_rays_occ): one workgroup per CU whatever
// the count (it is read on the device; the host never learns it), capped by the blocks the list can
// hold at most.
int launch_mlp16s_live(const float* packed, const float* o, const float* d, const float* z, int64_t R, int N,
                       const float* feat, float* rgb, float* sigma, const int* live, const int* live_count,
                       hipStream_t s) {
  const int64_t M = R * (int64_t)N;
  if (M == 0) return NERF_OK;
  constexpr int per_block = 32 * kW16Waves;
  const int64_t blocks = (M + per_block - 1) / per_block;
  const int cus = device_cus();
  if (cus <= 0) return set_error(NERF_ERR_HIP, "mlp16s_live_kernel: cannot read the device's CU count");
  const RayDiv nd = ray_div_of(N);
  hipLaunchKernelGGL(mlp16s_live_kernel, dim3((unsigned)(blocks < cus ? blocks : cus)), dim3(64 * kW16Waves), 0, s,
                     packed, o, d, z, N, feat, rgb, sigma, live, live_count, nd.mul, nd.shift);
  return check_launch("mlp16s_live_kernel");
}

}  // namespace nerf
