// The render MLP's kernel (mlp16s.hip, which describes it), included there twice:
//   MLP16S_GATHER 0: mlp16s_kernel, the samples 0 .. M-1 of the (R, N) launch;
//   MLP16S_GATHER 1: mlp16s_live_kernel, the M = *live_count samples named by the ascending list
//     `live` (sample r N + s).  Position i of the list takes the place of sample i wherever a block
//     is formed; the sample's ray, z, feature row and output row follow from live[i].  Rows outside
//     the list are not written.
// The plain entry's text is kept free of the variant (preprocessor branches, not a template over
// the body): its generated code is the one bench.py measures and check_isa.py addresses by name,
// and it does not change with this file's second inclusion.
__global__ void __launch_bounds__(64 * kW16Waves, 1)
#if MLP16S_GATHER
mlp16s_live_kernel(const float* __restrict__ packed, const float* __restrict__ orig, const float* __restrict__ dirs,
                   const float* __restrict__ zv, int N, const float* __restrict__ feat, float* __restrict__ rgb,
                   float* __restrict__ sigma, const int* __restrict__ live, const int* __restrict__ live_count,
                   uint32_t n_mul, int n_shift) {
#else
mlp16s_kernel(const float* __restrict__ packed, const float* __restrict__ orig, const float* __restrict__ dirs,
              const float* __restrict__ zv, int64_t M, int N, const float* __restrict__ feat,
              float* __restrict__ rgb, float* __restrict__ sigma, const int* __restrict__ out_slot, int out_T,
              uint32_t n_mul, int n_shift) {
#endif
  __shared__ __attribute__((aligned(16))) float lds[kSLdsFloats + kSStampFloats];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane0 = threadIdx.x & 63;
#if MLP16S_GATHER
  // the count is the device's: a workgroup with no block of its own leaves before any barrier
  // (count = 0 included, where mlast would be -1)
  const int64_t M = *live_count;
  if ((int64_t)blockIdx.x * (32 * kW16Waves) >= M) return;
  const int* const out_slot = nullptr;
  constexpr int out_T = 0;
#endif
  // every wave runs to the end (the weight stream has barriers); tail lanes repeat sample M-1.  A
  // launch spans < 2^31 samples (capi.hip max_launch_samples): 32-bit sample and ray indices.
  const int mlast = (int)(M - 1);
  // The workgroup runs sample blocks blockIdx.x, blockIdx.x + gridDim.x, ...: the trip count depends
  // on blockIdx.x alone, so the four waves run the same barriers.
  const int nblk = (int)((M + 32 * kW16Waves - 1) / (32 * kW16Waves));
  int blk = blockIdx.x;
  // (unsigned: the block one past the end may pass 2^31 before the clamp)
  auto sample_of = [&](int b, int st) {
    const uint32_t i = ((uint32_t)b * kW16Waves + wave) * 32 + 16 * st + (lane0 & 15);
    return (int)(i < (uint32_t)mlast ? i : (uint32_t)mlast);
  };
  // a sample's ray, sm / N: one multiply-high by the host's reciprocal of N (sample_index.h), no
  // division in the block loop
  auto ray_of = [&](int sm) {
#ifdef NERF16S_DIV_INDEX   // (A/B build: the compiler's division)
    return sm / N;
#else
    return ray_div(sm, n_mul, n_shift);
#endif
  };
  // cst / s for a scale s of pow2_scale's: s is a power of two, the product by its exact reciprocal is
  // the same correctly rounded value as the IEEE division's eleven instructions
  auto over_scale = [](float c, float s) {
#ifdef NERF16S_IEEE_INV   // (A/B build: the division)
    return c / s;
#else
    return c * pow2_recip(s);
#endif
  };
  // a block's inputs as loaded (SIn) and its sample positions from them.  The loads carry no branch
  // on zv (a branch behind a publish splits the block loop's body and waits for its loads on the
  // spot): without z values (points, row = sample) z and the directions are read from `orig`, which
  // holds a row per sample then, and positions() drops them.
  float in_z[2], in_o[2][3], in_d[2][3];
  const int pt_mask = zv ? 0 : -1;
  const float* const z_or = zv ? zv : orig;
  const float* const d_or = zv ? dirs : orig;
#if MLP16S_GATHER
  // the block's samples (sm_cur) and the next block's (sm_n), read from the live list at the
  // positions sample_of gives
  int sm_cur[2], sm_n[2];
  auto load_live = [&](int b, int (&sm)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 2; ++st) sm[st] = live[sample_of(b, st)];
  };
  auto load_inputs = [&](const int (&sml)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int sm = sml[st];
#else
  auto load_inputs = [&](int b) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int sm = sample_of(b, st);
#endif
      const int64_t row = (ray_of(sm) & ~pt_mask) | (sm & pt_mask);   // the sample's ray, or the point itself
#pragma unroll
      for (int c = 0; c < 3; ++c) in_o[st][c] = orig[3 * row + c];
      in_z[st] = z_or[sm];
#pragma unroll
      for (int c = 0; c < 3; ++c) in_d[st][c] = d_or[3 * row + c];
    }
  };
  float x[2][3];
  auto positions = [&](float (&x)[2][3]) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int c = 0; c < 3; ++c) {   // pts = o + d*z with separate roundings (ray_utils.py:86)
        const float p = in_o[st][c] + in_d[st][c] * in_z[st];
        x[st][c] = pt_mask ? in_o[st][c] : p;
      }
  };
#if MLP16S_GATHER
  load_live(blk, sm_cur);
  load_inputs(sm_cur);
#else
  load_inputs(blk);
#endif
  positions(x);
  // once per workgroup: biases, density head, layer constants and the rgb head into LDS
  for (int i = threadIdx.x; i < kSLdsVecFloats / 4; i += 64 * kW16Waves)
    reinterpret_cast<f32x4*>(lds + kSLdsBias)[i] = reinterpret_cast<const f32x4*>(packed + kOffBias)[i];
  if (threadIdx.x < kS16Consts) lds[kSLdsConsts + threadIdx.x] = packed[kOffScale16 + threadIdx.x];
  if (threadIdx.x < kSLdsRgbFloats / 4)
    reinterpret_cast<f32x4*>(lds + kSLdsRgb)[threadIdx.x] = reinterpret_cast<const f32x4*>(packed + kOffRgbW)[threadIdx.x];
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_sched_barrier(0);
  const float* stream = packed + kOff16;
  uint32_t lds_dma = (uint32_t)(uintptr_t)(lptr_t)lds + kSDmaWave * wave;
  // fragment offsets: row half r, lane l reads piece (g >> 1) lane R_r(l & 15) + 32 (g & 1)
  auto fragment_offsets = [](int l, uint32_t (&off)[2]) __attribute__((always_inline)) {
    const int li = l & 15, hh = (l >> 4) & 1, ss = l >> 5;
#pragma unroll
    for (int r = 0; r < 2; ++r) off[r] = (uint32_t)(ss * 2048 + 4 * ((li & 7) + 8 * r + 16 * (li >> 3) + 32 * hh));
  };
  float* pe_mine = lds + kSLdsPe + wave * kPeSteps * 64;
  const float* bias = lds + kSLdsBias;
  const float* ws = lds + kSLdsSigmaW;
  const float* cst = lds + kSLdsConsts;
#if MLP16S_GATHER
  constexpr bool one_ray = false;   // a wave's live samples lie on any rays: the per-sample feature rows
#else
  const bool one_ray = (N & 31) == 0;
#endif
  float* feat_mine = lds + kSLdsFeat + wave * kRayFeat;
  // the first block's chunks 0-2 and its chunk 0's tiles 0-2 (chunks 1-2 in flight); later blocks get
  // theirs from the colour layer of the block before
  STile a[4];
  {
    const uint32_t voff = 16u * lane0 + kSDmaWave * wave;
    sdma_chunk<0>(stream, 0, lds_dma, voff);
    sdma_chunk<1>(stream, 1, lds_dma, voff);
    sdma_chunk<2>(stream, 2, lds_dma, voff);
    uint32_t off[2];
    fragment_offsets(lane0, off);
    wait_vmcnt<8>();
    __builtin_amdgcn_s_barrier();
    sread_tile<0>(lds, off, a[0]);
    sread_tile<1>(lds, off, a[1]);
    sread_tile<2>(lds, off, a[2]);
  }

  Operand pe_op[4];   // layer 0's (and, re-split, the skip layer's) PE operands: [t][st] -> 2 t + st
  bool full = true;   // this block's encoding is still to be computed
#ifdef NERF_MLP16S_STAMPS
  int it = 0;
#endif
#pragma unroll 1
  for (;;) {
  // The stream's base, the ring's LDS address and the lane are opaque to the compiler per block:
  // otherwise it hoists every chunk's piece addresses and every per-lane LDS address and PE constant
  // (loop-invariant, over a hundred registers) out of the block loop and spills.  What derives from
  // the lane (a dozen VALU instructions) is therefore computed per block.
  asm volatile("" : "+s"(stream));
  asm volatile("" : "+s"(lds_dma));
  int lane = lane0;
  asm volatile("" : "+v"(lane));
  const int g = lane >> 4, li = lane & 15, hh = g & 1, ss = g >> 1;
  const uint32_t voff = 16u * lane + kSDmaWave * wave;
  uint32_t off[2];
  fragment_offsets(lane, off);
  const int nlane = 4 * hh + 16 * ss;   // this lane's neuron offset in a 16 x 16 output tile (+ 8r + e)
#ifdef NERF_MLP16S_STAMPS
  const bool stamp_on = it == kSStampIter || (it < kSStampIter && blk + (int)gridDim.x >= nblk);
  ++it;
#endif
  STAMP16S(0);
  STAMP16S_REAL(12);
  const uint32_t s0 = ((uint32_t)blk * kW16Waves + wave) * 32;

  // PE: lane group g = 2s + h computes slots 8 (2t + s) + j (t = 0, 1) of both its samples, sin for
  // h = 0 and cos for h = 1 (pe_feature; slot 30: x0 | x1, 31: x2 | 0).  Slot p < 30 is frequency
  // p / 3 of coordinate p % 3.  A wave with a coordinate beyond pe_sin.h's range takes sincosf.
  // The block before computed this block's encoding and layer-0 operands in its MFMA shadow (side_pe_next
  // below); only the workgroup's first block and a wave with such a coordinate (`full`) do it here.
  auto pe_arg = [&](const float (&xa)[2][3], int st, int p) __attribute__((always_inline)) {
    const int fi = p / 3, fc = p - 3 * fi;
    const float xc = fc == 0 ? xa[st][0] : (fc == 1 ? xa[st][1] : xa[st][2]);
    return xc * __int_as_float((127 + (fi < kPosLevels ? fi : 0)) << 23);   // x 2^fi, exact
  };
  auto pe_tail = [&](const float (&xa)[2][3], int st, int p, float v) __attribute__((always_inline)) {
    return p < 3 * kPosLevels ? v : (p == 30 ? (hh ? xa[st][1] : xa[st][0]) : (hh ? 0.0f : xa[st][2]));
  };
  auto pe_beyond = [&](const float (&xa)[2][3]) __attribute__((always_inline)) {
    float ax = 0.0f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
      ax = fmaxf(ax, fmaxf(fabsf(xa[st][0]), fmaxf(fabsf(xa[st][1]), fabsf(xa[st][2]))));
    return __any(ax * (float)(1 << (kPosLevels - 1)) > kPeSinMax) != 0;
  };
  auto pe_bound = [&](const float (&xa)[2][3], int st) __attribute__((always_inline)) {
    return fmaxf(1.0f, fmaxf(fabsf(xa[st][0]), fmaxf(fabsf(xa[st][1]), fabsf(xa[st][2]))));
  };
  float m_pe[2];
  float s_cur[2], inv_cur[2], s_nxt[2], inv_prev[2], m[2] = {0.0f, 0.0f}, part[2] = {0.0f, 0.0f};
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    m_pe[st] = pe_bound(x, st);
    s_cur[st] = pow2_scale(m_pe[st]);
  }
  if (full) {
    float pe[2][2][8];
    if (pe_beyond(x)) {
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int p = 8 * (2 * t + ss) + j;
            float sn, cs;
            sincosf(pe_arg(x, st, p), &sn, &cs);
            pe[st][t][j] = pe_tail(x, st, p, hh ? cs : sn);
          }
    } else {
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int p = 8 * (2 * t + ss) + j;
            pe[st][t][j] = pe_tail(x, st, p, pe_sin_reduced(pe_arg(x, st, p), hh));
          }
    }
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          pe_mine[((st * 2 + t) * 8 + j) * 64 + lane] = pe[st][t][j];
          split_into(pe[st][t][j] * s_cur[st], pe_op[2 * t + st], j);
        }
  }
  // the next block (one past the end repeats sample M-1): its inputs are loaded behind a publish of
  // layer 7's group A, and its encoding runs in the segments of layer 7's group B and of the colour
  // layer that carry no quarter, one value each, written to the wave's LDS copy (dead since layer 4)
  // and split into pe_op at the next block's layer-0 scale
  const int nxt_blk = blk + (int)gridDim.x;
  float xn[2][3], s_n[2];
  bool beyond_n = false;
  Operand pe_nx[4];   // (its own registers: pe_op's hold the skip layer's re-split until layer 4 ends)
  // (the lane once more opaque: otherwise every slot's frequency and coordinate select, shared with
  // the code above, stays in registers from there to here)
  int lane_n = lane;
  auto pub_next = [&](auto ic) __attribute__((always_inline)) {
#if MLP16S_GATHER
    // the dependent loads a chunk-step apart, each right behind a publish (where a wait for the
    // kernel's own loads costs next to nothing): the indices, then the inputs they name
    if constexpr (decltype(ic)::value == 0) load_live(nxt_blk, sm_n);
    if constexpr (decltype(ic)::value == 1) load_inputs(sm_n);
    if constexpr (decltype(ic)::value == 3) {
#else
    if constexpr (decltype(ic)::value == 0) load_inputs(nxt_blk);
    if constexpr (decltype(ic)::value == 2) {
#endif
      asm volatile("" : "+v"(lane_n));
      // (the loaded inputs opaque until here: otherwise their positions are computed, and the loads
      // waited for, right behind the loads' issue)
#pragma unroll
      for (int st = 0; st < 2; ++st)
        asm volatile("" : "+v"(in_z[st]), "+v"(in_o[st][0]), "+v"(in_o[st][1]), "+v"(in_o[st][2]), "+v"(in_d[st][0]),
                     "+v"(in_d[st][1]), "+v"(in_d[st][2]));
      positions(xn);
#pragma unroll
      for (int st = 0; st < 2; ++st) s_n[st] = pow2_scale(pe_bound(xn, st));
      beyond_n = pe_beyond(xn);
    }
  };
  auto side_pe_next = [&](auto nc, auto ph) __attribute__((always_inline)) {
    constexpr int n = decltype(nc)::value;
    if constexpr (n >= 0 && decltype(ph)::value == 1) {
      constexpr int st = n >> 4, t = (n >> 3) & 1, j = n & 7;
      // the lane's slot is 16 t + j (lane groups 0, 1) or 16 t + 8 + j (groups 2, 3): both slots'
      // frequency and coordinate are compile-time, one select picks the lane's (no branch, and the
      // same exact product x 2^f as pe_arg)
      constexpr int p0 = 16 * t + j, p1 = p0 + 8;
      constexpr int f0 = p0 / 3, c0 = p0 % 3, f1 = p1 / 3 < kPosLevels ? p1 / 3 : 0, c1 = p1 % 3;
      const bool upper = lane_n >= 32;
      const int hn = (lane_n >> 4) & 1;
      const float a0 = xn[st][c0] * (float)(1 << f0), a1 = xn[st][c1] * (float)(1 << f1);
      const float r = pe_sin_reduced(upper ? a1 : a0, hn);
      float v = r;
      if constexpr (p1 == 30) v = upper ? (hn ? xn[st][1] : xn[st][0]) : r;
      if constexpr (p1 == 31) v = upper ? (hn ? 0.0f : xn[st][2]) : r;
      pe_mine[((st * 2 + t) * 8 + j) * 64 + lane_n] = v;
      split_into(v * s_n[st], pe_nx[2 * t + st], j);
      // (the operand materialised here: otherwise the compiler keeps v to convert it in a pair with
      // the next segment's value)
      asm volatile("" : "+v"(pe_nx[2 * t + st].hi), "+v"(pe_nx[2 * t + st].lo));
    }
  };
  SAcc acc;
  Operand in[16];
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    inv_cur[st] = over_scale(cst[kS16InvW + 0], s_cur[st]);
    s_nxt[st] = pow2_scale(cst[kS16R + 0] * m_pe[st] + cst[kS16B + 0]);
  }
  SQuarter qv[2];
  SHalf hv[2];
  float pe_v[8];
  auto pe_operand_of = [&](auto i, auto st) -> const Operand& {
    return pe_op[2 * decltype(i)::value + decltype(st)::value];
  };

  STAMP16S(1);
  // ---- layer 0: PE (2 k-steps of 32) -> 256; group B converts group A's tiles 0-3 into in[0..7],
  // two quarters per segment
  sgroup<0, 2, 0, 3, kSNone>(stream, 0, lds, lds_dma, voff, off, a, acc, pe_operand_of,
                             [](auto, auto, auto) {});
  sgroup<1, 2, 2, 3, kSL0>(stream, 2, lds, lds_dma, voff, off, a, acc, pe_operand_of,
                           [&](auto i, auto seg, auto ph) __attribute__((always_inline)) {
                             constexpr int q0 = 8 * decltype(i)::value + 2 * decltype(seg)::value;
                             squarter<decltype(ph)::value, 0, q0, false>(acc, inv_cur, bias, ws, nlane, s_nxt, in, m,
                                                                         part, qv[0]);
                             squarter<decltype(ph)::value, 0, q0 + 1, false>(acc, inv_cur, bias, ws, nlane, s_nxt, in,
                                                                             m, part, qv[1]);
                           });

  STAMP16S(2);
  // ---- layers 1..7 (mlp16's schedule; on entry in[0..7] hold y_{L-1} tiles 0-3 at s_cur, its tiles
  // 4-7 wait in acc[4..7], m the sample tiles' maxima of y_{L-1} tiles 0-3)
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    inv_prev[st] = inv_cur[st];
    s_cur[st] = s_nxt[st];
  }
  const float* bias_prev = bias;
  auto act_operand = [&](auto i, auto st) -> const Operand& { return in[2 * decltype(i)::value + decltype(st)::value]; };
  auto op4 = [&](auto i, auto st) -> const Operand& {
    constexpr int k = decltype(i)::value, t = decltype(st)::value;
    if constexpr (k < 8) return in[2 * k + t];
    else return pe_op[2 * (k - 8) + t];
  };
  auto side_prev = [&](auto i, auto seg, auto ph, auto sigma_tag) __attribute__((always_inline)) {
    constexpr int q = sq_prev(decltype(i)::value, decltype(seg)::value);
    if constexpr (q >= 0)
      squarter<decltype(ph)::value, 4, q, decltype(sigma_tag)::value>(acc, inv_prev, bias_prev, ws, nlane, s_cur, in, m,
                                                                       part, qv[0]);
  };
  auto side_cur = [&](auto i, auto seg, auto ph, const float* bias_l, auto sigma_tag) __attribute__((always_inline)) {
    constexpr int q = sq_cur(decltype(i)::value, decltype(seg)::value);
    if constexpr (q >= 0)
      squarter<decltype(ph)::value, 0, q, decltype(sigma_tag)::value>(acc, inv_cur, bias_l, ws, nlane, s_nxt, in, m,
                                                                      part, qv[1]);
  };
  // the plain trunk's sides in half-quarters, a unit per MFMA gap (ssegment_h; slot: the segment's
  // first or second half)
  auto side_prev_h = [&](auto i, auto seg, auto slot, auto unit) __attribute__((always_inline)) {
    constexpr int h = sh_prev(decltype(i)::value, decltype(seg)::value, decltype(slot)::value);
    if constexpr (h >= 0 && decltype(unit)::value >= -1)
      shalf<decltype(unit)::value, 4, h>(acc, inv_prev, bias_prev, nlane, s_cur, in, m, hv[decltype(slot)::value]);
    if constexpr (decltype(slot)::value == 1 && h >= 0)
      shalf_follow<decltype(unit)::value>(hv[0], hv[1]);
  };
  auto side_cur_h = [&](auto i, auto seg, auto slot, auto unit, const float* bias_l) __attribute__((always_inline)) {
    constexpr int h = sh_cur(decltype(i)::value, decltype(seg)::value, decltype(slot)::value);
    if constexpr (h >= 0 && decltype(unit)::value >= -1)
      shalf<decltype(unit)::value, 0, h>(acc, inv_cur, bias_l, nlane, s_nxt, in, m, hv[decltype(slot)::value]);
    if constexpr (decltype(slot)::value == 1 && h >= 0)
      shalf_follow<decltype(unit)::value>(hv[0], hv[1]);
  };
#ifdef NERF16S_QUARTER_SIDE   // (A/B build: the quarter schedule in the plain trunk too)
  constexpr int kKindPrev = kSPrev, kKindCur = kSCur;
#else
  constexpr int kKindPrev = kSPrevH, kKindCur = kSCurH;
#endif
  // the skip layer's PE operands at layer 4's input scale (s_cur in group A, which group B keeps)
  float s_pe[2] = {0.0f, 0.0f};
  auto side_pe = [&](auto i, auto seg, auto ph) __attribute__((always_inline)) {
    constexpr int k = spe_at(decltype(i)::value, decltype(seg)::value);
    if constexpr (k >= 0) spe_operand<decltype(ph)::value, k / 2, k % 2>(pe_mine, s_pe, pe_op[k], pe_v, lane);
  };
  using NoSigma = std::false_type;
  using Sigma = std::true_type;
  // one trunk layer (SKIP: layer 4 reads [h3, enc_x], 10 chunk-steps per group; SG: layer 7 starts the
  // density head).  Layers 1-3 and 5-6 run as loops of the plain body, layers 4 and 7 on their own:
  // one body with the skip and sigma variants behind runtime branches spilled (the register
  // allocator then has to serve every variant's live ranges at the loop's back edge).
  auto layer = [&](int L, auto skip_tag, auto sg_tag, auto&& pub_a) __attribute__((always_inline)) {
    constexpr bool SKIP = decltype(skip_tag)::value;
    constexpr bool SG = decltype(sg_tag)::value;
    sacc_hold(acc);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      inv_cur[st] = over_scale(cst[kS16InvW + L], s_cur[st]);
      if constexpr (SKIP) s_pe[st] = s_cur[st];
    }
    const float* bias_l = bias + L * kHidden;
    const int c0 = s16_chunk0(1) + (L - 1) * 16 + (L > kSkipLayer ? 4 : 0);
    if constexpr (SKIP) {
      // layer 4 reads [h3, enc_x]: its PE operands (k-steps 8, 9) are split just before they are read
      sgroup<0, 10, 0, 3, kSSkipPrev>(stream, c0, lds, lds_dma, voff, off, a, acc, op4,
                                      [&](auto i, auto seg, auto ph) __attribute__((always_inline)) {
                                        side_prev(i, seg, ph, NoSigma{});
                                        side_pe(i, seg, ph);
                                      });
    } else {
      sgroup<0, 8, 0, 3, kKindPrev>(stream, c0, lds, lds_dma, voff, off, a, acc, act_operand,
                                    [&](auto i, auto seg, auto... at) __attribute__((always_inline)) {
                                      if constexpr (sizeof...(at) == 2) side_prev_h(i, seg, at...);
                                      else side_prev(i, seg, at..., NoSigma{});
                                    }, pub_a);
    }
    // the inputs of layer L are known: the scale of layer L+1's inputs from the bound on y_L
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const float ms = smax4(m[st]);
      float bound = cst[kS16R + L] * (SKIP ? fmaxf(ms, m_pe[st]) : ms) + cst[kS16B + L];
      if (L + 1 == kSkipLayer) bound = fmaxf(bound, m_pe[st]);    // layer 4 splits the PE at the same scale
      s_nxt[st] = pow2_scale(bound);
      m[st] = 0.0f;
    }
    if constexpr (SKIP) {
      sgroup<1, 10, 2, 3, kSSkipCur>(stream, c0 + 10, lds, lds_dma, voff, off, a, acc, op4,
                                     [&](auto i, auto seg, auto ph) __attribute__((always_inline)) {
                                       side_cur(i, seg, ph, bias_l, NoSigma{});
                                       side_pe(i, seg, ph);
                                     });
    } else {
      // (layer 7, SG: the next block's encoding in the free segments)
      sgroup<1, 8, 0, 3, SG ? kSCurPe : kKindCur>(
          stream, c0 + 8, lds, lds_dma, voff, off, a, acc, act_operand,
          [&](auto i, auto seg, auto... at) __attribute__((always_inline)) {
            if constexpr (sizeof...(at) == 2) {
              side_cur_h(i, seg, at..., bias_l);
            } else {
              side_cur(i, seg, at..., bias_l, sg_tag);
              if constexpr (SG)
                side_pe_next(std::integral_constant<int, spe_next<true>(decltype(i)::value, decltype(seg)::value)>{},
                             at...);
            }
          });
    }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      inv_prev[st] = inv_cur[st];
      s_cur[st] = s_nxt[st];
    }
    bias_prev = bias_l;
    STAMP16S(2 + L);
  };
#pragma unroll 1
  for (int L = 1; L < kSkipLayer; ++L) layer(L, NoSigma{}, NoSigma{}, SNoPub{});
  layer(kSkipLayer, Sigma{}, NoSigma{}, SNoPub{});
#pragma unroll 1
  for (int L = kSkipLayer + 1; L < 7; ++L) layer(L, NoSigma{}, NoSigma{}, SNoPub{});
  layer(7, NoSigma{}, Sigma{}, pub_next);

  // ---- colour layer: h7 -> 128 (one group of 8 chunks); its side converts y_7 tiles 4-7 and
  // finishes the density head.  The stream wraps: the layer's chunk-steps DMA the next block's chunks
  // 0-2, publish chunk 0 and read its tiles 0-2, which is where layer 0 starts (after the workgroup's
  // last block those chunks are fetched for nothing, once per workgroup).  When N is a multiple of 32
  // the wave's samples lie on one ray: its 1 KiB of ray features is DMA'd into LDS meanwhile; it is
  // older than the wrapped chunks' pieces, so the layer's publishes cover it.
  // The DMA is issued whatever N is (a wave that spans rays reads its rows from memory below and
  // leaves the copy unused: the row of its first sample's ray is a valid one): a branch here ends
  // the basic block, and the compiler sinks what only the colour layer and the heads read (the density
  // head's 64 partial products, the next block's scales) out of layer 7's MFMA shadow into the
  // block behind it, with the registers that keeps alive saved and restored around the branch.
#if MLP16S_GATHER
  if (one_ray) {
#elif defined(NERF16S_DMA_BRANCH)   // (A/B build: the DMA only when it is used)
  if (one_ray) {
#else
  {
#endif
    const int first = (int)(s0 < (uint32_t)mlast ? s0 : (uint32_t)mlast);
    const char* src = reinterpret_cast<const char*>(feat + (int64_t)ray_of(first) * kRayFeat);
    const uint32_t dst = (uint32_t)(uintptr_t)(lptr_t)feat_mine;
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(16u * lane), "s"(src), "s"(dst)
        : "memory");
  }
  sacc_hold(acc);
#pragma unroll
  for (int st = 0; st < 2; ++st) inv_cur[st] = over_scale(cst[kS16InvW + 8], s_cur[st]);
  sgroup<0, 8, 0, 3, kSPrevPe, true>(
      stream, s16_chunk0(8), lds, lds_dma, voff, off, a, acc, act_operand,
      [&](auto i, auto seg, auto ph) __attribute__((always_inline)) {
        side_prev(i, seg, ph, Sigma{});
        side_pe_next(std::integral_constant<int, spe_next<false>(decltype(i)::value, decltype(seg)::value)>{}, ph);
      });

  STAMP16S(10);
  // density head: sigma = ReLU(density_head(ReLU(h7))) (models.py:137-138), f32
  float sig[2];
#pragma unroll
  for (int st = 0; st < 2; ++st) sig[st] = fmaxf(ssum4(part[st]) + ws[kHidden], 0.0f);
  // colour branch: h_dir = ReLU(W_dh ReLU(h7) + [b_dir + W_dd PE(d)]) + appearance (models.py:141-156)
  const float* wr = lds + kSLdsRgb;
  float pr[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  auto colour_head = [&](const float* fr, int st) __attribute__((always_inline)) {
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int n0 = 32 * T + 8 * r + nlane;
        const f32x4 fd = *reinterpret_cast<const f32x4*>(fr + n0);
        const f32x4 ap = *reinterpret_cast<const f32x4*>(fr + kDirHidden + n0);
        f32x4 hd;
#pragma unroll
        for (int e = 0; e < 4; ++e) hd[e] = fmaxf(fmaf(acc[T][r][st][e], inv_cur[st], fd[e]), 0.0f) + ap[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(wr + c * kDirHidden + n0);
#pragma unroll
          for (int e = 0; e < 4; ++e) pr[st][c] = fmaf(w[e], hd[e], pr[st][c]);
        }
      }
  };
  if (one_ray) wait_vmcnt<8>();   // the feature piece (younger: the next block's chunks 1-2)
  if (one_ray) {
    colour_head(feat_mine, 0);
    colour_head(feat_mine, 1);
  } else {
#if MLP16S_GATHER
    colour_head(feat + (int64_t)ray_of(sm_cur[0]) * kRayFeat, 0);
    colour_head(feat + (int64_t)ray_of(sm_cur[1]) * kRayFeat, 1);
#else
    colour_head(feat + (int64_t)ray_of(sample_of(blk, 0)) * kRayFeat, 0);
    colour_head(feat + (int64_t)ray_of(sample_of(blk, 1)) * kRayFeat, 1);
#endif
  }
  // Lane group st (0, 1) writes sample tile st.  Every lane holds both tiles' sums, but evaluates the
  // sigmoid, a double-precision exp, only for the tile its group writes (groups 2, 3 mirror 0, 1):
  // +0.5 % frame rate on the one-block kernel, same box (profiles/r07/ab_render_stage2_heads_gap.log).
  float out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v0 = ssum4(pr[0][c]) + wr[3 * kDirHidden + c], v1 = ssum4(pr[1][c]) + wr[3 * kDirHidden + c];
    const float v = (g & 1) ? v1 : v0;
    out[c] = 1.0f / (1.0f + expf_rn(-v));                              // sigmoid (models.py:159-160)
  }
  // lane group st writes sample tile st
  if (g < 2) {
    const int st = g;
    if (s0 + 16 * st + li <= (uint32_t)mlast) {
#if MLP16S_GATHER
      const int sm = st ? sm_cur[1] : sm_cur[0];
#else
      const int sm = (int)(s0 + 16 * st + li);
#endif
      const int64_t o_s = out_slot ? (int64_t)ray_of(sm) * out_T + out_slot[sm] : (int64_t)sm;
      sigma[o_s] = st ? sig[1] : sig[0];
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[3 * o_s + c] = out[c];
    }
  }
  STAMP16S(11);
  STAMP16S_REAL(13);
  if (nxt_blk >= nblk) break;
  blk = nxt_blk;
  full = beyond_n;
#pragma unroll
  for (int k = 0; k < 4; ++k) pe_op[k] = pe_nx[k];
#pragma unroll
  for (int st = 0; st < 2; ++st)
#pragma unroll
    for (int c = 0; c < 3; ++c) x[st][c] = xn[st][c];
#if MLP16S_GATHER
  sm_cur[0] = sm_n[0];
  sm_cur[1] = sm_n[1];
#endif
  }
  wait_vmcnt<0>();   // the wrapped stream's chunks 0-2 after the last block: nothing outstanding at the end
#ifdef NERF_MLP16S_STAMPS
  if (const int64_t w_ = (int64_t)blockIdx.x * kW16Waves + wave; w_ < 65536 && lane0 == 0)
    for (int i = 0; i < 16; ++i)
      nerf16s_stamps[w_][i] = reinterpret_cast<const unsigned long long*>(lds + kSLdsFloats)[wave * 16 + i];
#endif
}
