// Pixel-wise chain across a residual-block boundary of the ResNet trunk (reference graph:
// relation_rcnn/symbols/resnet_v1_101_rcnn_base.py, e.g. res2a_branch2c .. res2b_branch2a, :66-84):
//
//     x_next = relu(W3 . mid2 + b3 + x)            1x1 expand (BN folded) + identity shortcut + ReLU of block n
//     mid1'  = relu(W1' . x_next + b1')            1x1 reduce (BN folded) + ReLU of block n+1
//
// Both are 1x1 convolutions, i.e. per-pixel products, so block n+1's reduce can consume x_next while it is still in
// registers: the 256- (512-) channel activation is written once and NOT read back by a separate reduce kernel.  For the
// HBM-bound stages that is the dominant saving (res2 at B = 54: expand 535 us + reduce 256 us as two GEMM launches ->
// 461 us; DESIGN.md section 4 / 4a have the measured figures).  The same kernel without the second product is the
// expand + shortcut + ReLU layer of every residual unit (res2 .. res5), bit-identical to the implicit-GEMM launch.
//
// One wavefront = 32 pixels, in passes of 64 output channels:
//   phase A  acc^T[cout][px] = W3 (A operand, rows = cout, fragments from LDS) x mid2^T (B operand: lane = pixel, 8 channels
//            per k-step, read straight from HBM once per tile and kept in VGPRs);
//   shortcut the 32 px x 64-channel slice of x arrives in LDS by global_load_lds (1 KiB per instruction = 8 pixel rows of
//            128 B, 16-byte chunks XOR-swizzled on the SOURCE side so that the per-lane 8-byte reads spread over the banks),
//            one pass ahead; relu(acc + b3 + x) is written back IN PLACE as bf16 and leaves as 16-byte coalesced rows
//            one pass later;
//   phase B  the same packed bf16 values are the B operand of the second product (the contraction index cout is permuted
//            identically in the accumulator registers and in the pre-packed W1' fragments, as in the attention kernel),
//            mid1'^T[c][px] accumulates over the passes, then bias + ReLU + LDS transpose + coalesced rows.
// Rounding points are those of the two-launch path (x_next is rounded to bf16 before the reduce product).
#include "common.h"

namespace relnet {

typedef const __attribute__((address_space(1))) void* gas_ptr;
typedef __attribute__((address_space(3))) void* las_ptr;

// LDS-direct load issued from inline assembly: the compiler tracks no LDS-DMA store for it, so it does not put its own
// s_waitcnt vmcnt(0) in front of the next ds_read (which would drain the prefetched slices at once).  Ordering by hand at the call
// sites: counted vmcnt + barrier before a read (same helper as in gemm.hip).
__device__ __forceinline__ void chain_glds16(const void* src, unsigned lds_byte_addr) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_byte_addr) : "memory", "m0");
}

struct ChainArgs {
  const unsigned short* m2;   // [P][MID]   3x3 output of block n (bf16)
  const unsigned short* x;    // [P][4 MID] shortcut = input of block n
  const uint4* w3f;           // W3 [4 MID][MID] in fragment order (relnet_pack_w_frag)
  const uint4* w1f;           // W1' [MID][4 MID], fragment order with the accumulator permutation (ops.pack_chain_w1)
  const float* b3;            // [4 MID]
  const float* b1;            // [MID]
  const unsigned short* xin;  // PROJ: [P][MID] input of the unit (its projection shortcut is computed here, no x operand)
  const uint4* wpf;           // PROJ: Wp [4 MID][MID] (branch1) in fragment order
  unsigned short* xn;         // [P][4 MID]
  unsigned short* m1;         // [P][MID]
  int P;
  int H, W, Ho, Wo;           // GATHER: the full map x addresses and the compact one (Ho = (H - 1) / 2 + 1, Wo likewise); P = B * Ho * Wo
  int dbg;                    // timing ablations of chain256_roles_kernel (relnet_chain_debug; results are then WRONG): 1 = half of the weight
                              // loads (W3 pieces and W1' register loads), 2 = no weight loads, 4 = no shortcut-slice loads, 8 = no global stores
};

// One kernel for both widths, in passes of 64 output channels of the expand product:
//   MID = 64  (res2, STREAM = false): W3 / W1' (32 KiB each) stay in LDS for the life of the workgroup and the eight
//             wavefronts run independently (no barrier after the weight load);
//   MID = 128 (res3, STREAM = true):  the weights (2 x 128 KiB) do not fit, so the workgroup walks the passes in lock step and
//             the pass's W3 / W1' slices (16 KiB each) go through a two-slot LDS ring, requested one pass ahead.
// Per wavefront the shortcut slice of pass p+1 (32 px x 64 channels, 4 KiB, second stage buffer) is requested and the
// finished slice of pass p-1 is stored BEFORE the arithmetic of pass p, so both are in flight during it; loads and stores
// share vmcnt and complete out of order with respect to each other, hence the single vmcnt(0) at the top of a pass.
// Nothing on the vector-memory path is issued inside the arithmetic (biases come from LDS): a load there would make the
// compiler wait for the prefetch in front of it.
// KSPLIT > 1 (MID = 512, res5; expand-only): the k range of a pass is cut in KSPLIT sub-steps so that a ring slot stays 32 KiB.
// (measured and dropped, r04: vector-memory roles per wavefront for this form -- four wavefronts stream weights, four move the activations
//  of all eight tiles, the mid-pass step only drains weight loads: 19.62 vs 19.59 ms per 54-image step, no gain; res5's expand is bound
//  by its 2 MB weight stream per 256 pixels through the L2 -> LDS fill path)
// MID = 256 with the second product (res4): chain256_roles_kernel below.
// GATHER (expand-only, MID = 64 / 128; the last unit of res2 / res3, whose output only the stride-2 1x1 layers of the next stage read):
//   mid2 and x_next are compact [B][Ho][Wo] maps of the even (y, x) pixels, the shortcut x stays the full [B][H][W] map and compact
//   pixel q = (b, yo, xo) reads it at (b H + 2 yo) W + 2 xo.  The four row offsets of a lane (rows 8 i + drow of the tile) are worked
//   out once per tile -- at the tile's last pass, for the tile after it -- and are the only per-lane address state (4 VGPRs, no
//   scratch: a reload in the pass loop would put a vmcnt(0) between the prefetches).  Passes, k order, rounding points, LDS stage
//   layout and stores are those of the dense form: the kept pixels carry the same bits.  Never in place (the shapes differ).
// PROJ (MID = 64, resident weights; the first unit of res2, whose shortcut is a 1x1 projection of the unit's 64-channel input):
//   x_next = relu(W3 . mid2 + Wp . x_in + (b3 + bp)) -- the projection is four more k-steps of the same accumulators instead of a
//   separate convolution that writes a 4 MID-channel map (1.04 GB at 54 images) for this kernel to read back; no shortcut slice,
//   one stage buffer per wave (written, then flushed in the same pass).  The shortcut is not rounded to bf16 on the way.
template <int MID, bool STREAM, bool REDUCE = true, int KSPLIT = 1, bool PROJ = false, bool GATHER = false>       // REDUCE = false: only x_next (no next reduce)
__global__ __launch_bounds__(512) void bottleneck_chain_kernel(ChainArgs a) {
  static_assert(!PROJ || (!STREAM && KSPLIT == 1), "the projection form exists for the resident-weight kernel");
  static_assert(!GATHER || (!REDUCE && !PROJ && KSPLIT == 1), "the stride-2 gather exists for the plain expand-only forms");
  static_assert(KSPLIT == 1 || (STREAM && !REDUCE), "k-split passes exist for the streamed expand-only form");
  constexpr int COUT = 4 * MID, KS = MID / 16, KSS = KS / KSPLIT, RT = MID / 32, NP = COUT / 64;
  static_assert(!REDUCE || MID <= 128, "MID = 256 with the second product is chain256_roles_kernel");
  constexpr int W3P = 2 * KSS * 1024, W1P = REDUCE ? 4 * RT * 1024 : 0;     // bytes of one (sub-)step's W3 / W1' slice
  constexpr int WPP = PROJ ? W3P : 0;                                         // ... and of its Wp slice
  constexpr int PASSB = W3P + WPP + W1P;
  constexpr int STG = PROJ ? 4096 : 8192;                                     // stage bytes per wave
  constexpr int WBYTES = STREAM ? 2 * PASSB : NP * PASSB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  unsigned char* stage = smem + WBYTES + wave * STG;           // 2 (PROJ: 1) x [32 px][128 B], chunk c of row r at c ^ ((r >> 1) & 7)
  float* sB3 = (float*)(smem + WBYTES + 8 * STG);              // [COUT]
  float* sB1 = sB3 + COUT;                                     // [MID]
  for (int i = tid; i < COUT; i += 512) sB3[i] = a.b3[i];
  if constexpr (REDUCE) for (int i = tid; i < MID; i += 512) sB1[i] = a.b1[i];
  if constexpr (!STREAM) {                                      // resident layout: pass-major, [pass][W3 slice | W1' slice]
    for (int i = tid; i < NP * PASSB / 16; i += 512) {
      const int p = i / (PASSB / 16), r = i % (PASSB / 16);
      uint4 v;
      if (r < W3P / 16) v = a.w3f[(long)p * (W3P / 16) + r];
      else if (r < (W3P + WPP) / 16) v = a.wpf[(long)p * (W3P / 16) + (r - W3P / 16)];
      else { const int q = (r - (W3P + WPP) / 16) >> 6, rt = q >> 2, kk = q & 3; v = a.w1f[((long)rt * (COUT / 16) + p * 4 + kk) * 64 + (r & 63)]; }
      ((uint4*)smem)[i] = v;
    }
  }
  __syncthreads();
  const int ntile = (a.P + 31) / 32;
  const int drow = lane >> 3, dslot = lane & 7;                // DMA / coalesced-store role: row 8 i + drow, chunk slot dslot
  // GATHER: byte offsets into x of the pixels that rows 8 i + drow of the tile at p0 read (clamped like the dense rows)
  unsigned xrow[GATHER ? 4 : 1];
  auto gather_rows = [&](int p0) {
    if constexpr (GATHER) {
      const unsigned hw = (unsigned)(a.Ho * a.Wo);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned q = (unsigned)min(p0 + 8 * i + drow, a.P - 1);
        const unsigned b = q / hw, r = q - b * hw, yo = r / (unsigned)a.Wo, xo = r - yo * (unsigned)a.Wo;
        xrow[i] = ((b * (unsigned)a.H + 2u * yo) * (unsigned)a.W + 2u * xo) * (COUT * 2u);
      }
    }
  };
  // shortcut slice of (tile base pixel p0, pass p) into stage buffer p & 1 (GATHER: of the tile gather_rows was last called for)
  auto issue_x = [&](int p0, int p) {
    if constexpr (PROJ) return;
    unsigned char* sb = stage + (p & 1) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 8 * i + drow;
      // (32-bit byte offsets from the tensor base -- the host checks P * COUT * 2 < 2^32: half the address registers per row)
      const unsigned off = GATHER ? xrow[i] + (p * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) * 2u
                                  : ((unsigned)min(p0 + row, a.P - 1) * COUT + p * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) * 2u;
      __builtin_amdgcn_global_load_lds((gas_ptr)((const unsigned char*)a.x + off), (las_ptr)(sb + i * 1024), 16, 0, 0);
    }
  };
  // (STREAM) this wave's share of the weights of step st = pass * KSPLIT + k-part into ring slot st & 1
  auto issue_w = [&](int st) {
    if constexpr (STREAM) {
      const int p = st / KSPLIT, kh = st % KSPLIT;
      unsigned char* wb = smem + (st & 1) * PASSB;
#pragma unroll
      for (int i = 0; i < (2 * KSS + (REDUCE ? 4 * RT : 0)) / 8; ++i) {
        const int q = wave + 8 * i;
        if (q < 2 * KSS) {
          const int ct = q / KSS, ks = q % KSS;
          __builtin_amdgcn_global_load_lds((gas_ptr)(a.w3f + ((long)((p * 2 + ct) * KS + kh * KSS + ks) * 64 + lane)), (las_ptr)(wb + q * 1024), 16, 0, 0);
        } else {
          const int q1 = q - 2 * KSS, rt = q1 >> 2, kk = q1 & 3;
          __builtin_amdgcn_global_load_lds((gas_ptr)(a.w1f + ((long)(rt * (COUT / 16) + p * 4 + kk) * 64 + lane)), (las_ptr)(wb + W3P + q1 * 1024), 16, 0, 0);
        }
      }
    }
  };
  // stores of a finished 32 px x 64 channel slice of x_next from stage buffer p & 1
  auto flush = [&](int p0, int p) {
    const unsigned char* sb = stage + (PROJ ? 0 : (p & 1) * 4096) + lane * 16;
    const uint4 v0 = *(const uint4*)sb, v1 = *(const uint4*)(sb + 1024), v2 = *(const uint4*)(sb + 2048), v3 = *(const uint4*)(sb + 3072);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    auto put = [&](int i, const uint4& v) {
      const int row = 8 * i + drow;
      if (p0 + row < a.P) *(uint4*)((unsigned char*)a.xn + ((unsigned)(p0 + row) * COUT + p * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) * 2u) = v;
    };
    put(0, v0); put(1, v1); put(2, v2); put(3, v3);
  };

  // tile sequence of this wavefront: independent tiles (resident) or lock-step sets of 8 tiles (streaming)
  const int t_first = blockIdx.x * 8 + wave;
  const int t_step = gridDim.x * 8;
  const int n_iter = STREAM ? ((ntile + 7) / 8 - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x
                            : (ntile - t_first + t_step - 1) / t_step;      // (streaming: idle waves of the last set still take part)
  if (n_iter <= 0) return;
  gather_rows(t_first * 32);
  issue_x(t_first * 32, 0);
  issue_w(0);
  for (int it = 0; it < n_iter; ++it) {
    const int p0 = (t_first + it * t_step) * 32;               // >= P for idle waves: loads clamp, stores are masked
    const int px = min(p0 + l31, a.P - 1);
    bf16x8 m2f[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) m2f[ks] = *(const bf16x8*)(a.m2 + (long)px * MID + 16 * ks + 8 * half);
    bf16x8 xf[PROJ ? KS : 1];
    if constexpr (PROJ) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(a.xin + (long)px * MID + 16 * ks + 8 * half);
    }
    f32x16 m1acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) m1acc[rt][r] = 0.f;
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {
      f32x16 acc[2];
#pragma unroll
      for (int kh = 0; kh < KSPLIT; ++kh) {
        const int st = p * KSPLIT + kh;
        if constexpr (STREAM) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");   // step st landed everywhere; everyone left step st-1
        else if constexpr (!PROJ) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (PROJ: no LDS-DMA in flight; its stores need no wait)
        if (kh == 0) {
          if (!PROJ && p > 0) flush(p0, p - 1);
          if (p + 1 < NP) issue_x(p0, p + 1);
          else if (it + 1 < n_iter) { gather_rows(p0 + t_step * 32); issue_x(p0 + t_step * 32, 0); }
        }
        if (st + 1 < NP * KSPLIT) issue_w(st + 1);
        else if (it + 1 < n_iter) issue_w(0);
        const uint4* w3 = (const uint4*)(smem + (STREAM ? (st & 1) : st) * PASSB);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          if (kh == 0)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KSS; ++ks)
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)&w3[(ct * KSS + ks) * 64 + lane], m2f[kh * KSS + ks], acc[ct], 0, 0, 0);
          if constexpr (PROJ) {
            const uint4* wp = (const uint4*)((const unsigned char*)w3 + W3P);
#pragma unroll
            for (int ks = 0; ks < KSS; ++ks)
              acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)&wp[(ct * KSS + ks) * 64 + lane], xf[ks], acc[ct], 0, 0, 0);
          }
        }
      }
      const uint4* w1 = (const uint4*)(smem + (STREAM ? (p & 1) : p) * PASSB + W3P + WPP);      // (REDUCE implies KSPLIT == 1: step == pass)
      unsigned char* sb = stage + (PROJ ? 0 : (p & 1) * 4096);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        // bias + shortcut + ReLU in place; the packed values feed the second product directly
        uint2 pk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          uint2* sp = (uint2*)(sb + l31 * 128 + (((ct * 4 + g) ^ ((l31 >> 1) & 7)) << 4) + 8 * half);
          const uint2 xv = PROJ ? make_uint2(0u, 0u) : *sp;
          const float4 bv = *(const float4*)(sB3 + p * 64 + ct * 32 + 8 * g + 4 * half);
          const float v0 = fmaxf(acc[ct][4 * g + 0] + bv.x + bf2f(xv.x & 0xffff), 0.f), v1 = fmaxf(acc[ct][4 * g + 1] + bv.y + bf2f(xv.x >> 16), 0.f);
          const float v2 = fmaxf(acc[ct][4 * g + 2] + bv.z + bf2f(xv.y & 0xffff), 0.f), v3 = fmaxf(acc[ct][4 * g + 3] + bv.w + bf2f(xv.y >> 16), 0.f);
          pk[g] = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
          *sp = pk[g];
        }
        if constexpr (REDUCE) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            bf16x8 xf;
            *(uint2*)&xf = pk[2 * j];
            *((uint2*)&xf + 1) = pk[2 * j + 1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
              m1acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)&w1[(rt * 4 + ct * 2 + j) * 64 + lane], xf, m1acc[rt], 0, 0, 0);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the slice is complete in LDS (same-wave readers only)
      __builtin_amdgcn_wave_barrier();
      if constexpr (PROJ) { flush(p0, p); __builtin_amdgcn_wave_barrier(); }      // single stage buffer: out before the next pass writes it
    }
    if constexpr (!PROJ) flush(p0, NP - 1);
    if constexpr (!REDUCE) continue;
    // mid1' = relu(. + b1), 64 channels at a time through the buffer that was just flushed (the other one is receiving
    // the next tile's first slice)
    unsigned char* sb = stage + (PROJ ? 0 : ((NP - 1) & 1) * 4096);
#pragma unroll
    for (int hc = 0; hc < RT / 2; ++hc) {
#pragma unroll
      for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int rt = 2 * hc + r2;
          const float4 bv = *(const float4*)(sB1 + rt * 32 + 8 * g + 4 * half);
          const float v0 = fmaxf(m1acc[rt][4 * g + 0] + bv.x, 0.f), v1 = fmaxf(m1acc[rt][4 * g + 1] + bv.y, 0.f);
          const float v2 = fmaxf(m1acc[rt][4 * g + 2] + bv.z, 0.f), v3 = fmaxf(m1acc[rt][4 * g + 3] + bv.w, 0.f);
          *(uint2*)(sb + l31 * 128 + (((r2 * 4 + g) ^ ((l31 >> 1) & 7)) << 4) + 8 * half) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      const unsigned char* sl = sb + lane * 16;
      const uint4 v0 = *(const uint4*)sl, v1 = *(const uint4*)(sl + 1024), v2 = *(const uint4*)(sl + 2048), v3 = *(const uint4*)(sl + 3072);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      auto put = [&](int i, const uint4& v) {
        const int row = 8 * i + drow;
        if (p0 + row < a.P) *(uint4*)(a.m1 + (long)(p0 + row) * MID + hc * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) = v;
      };
      put(0, v0); put(1, v1); put(2, v2); put(3, v3);
    }
  }
}




// ---------------------------------------------------------------------------------------------------------------------------
// res4 form of the two-product chain (MID = 256: 256 -> 1024 + shortcut + ReLU, then the next unit's 1024 -> 256 + ReLU), with ONE ROLE
// PER WAVEFRONT.  Every wavefront doing everything (bottleneck_chain_kernel's structure) needs 64 (mid2 fragments) + 128 (mid1'
// accumulators) + 16 registers of essential state per wavefront of 256 and spilled into the step loop (r04: 21.6 ms per 54-image step
// against 20.0 ms with roles).  Here a workgroup walks sets of FOUR 32-pixel tiles in lock step, one s_barrier per STEP = PASS = 64
// output channels of the expand product, 16 steps per set:
//   A-wave T (0..3)   tile T.  mid2 fragments once per tile (registers).  Step s: two independent accumulators (W3 rows [64 p, +32) and
//                     [64 p + 32, +32), fragments from the weight slot s & 1 in four batches through two register sets, ks = 0..15 each,
//                     MFMAs interleaved, at raised priority on the pipe the wave shares with a B-wave), bias + shortcut + ReLU of
//                     both halves in place into the tile's stage buffer s % 4, then the finished slice of pass s - 1 (fenced by the barrier
//                     at the top of the step; the B-waves only read it) goes out as 16-byte coalesced rows.  The stores drain in the
//                     background: an A-wave waits on vmcnt only for its mid2 fragments, once per tile.
//   B-wave b (4 + b)  mid1' channels [64 b, +64) of ALL FOUR tiles: 4 tiles x 2 row tiles x 16 accumulator registers.  Step s consumes
//                     pass s - 1: the slices the A-waves finished before the barrier, read back from the four stage rings, x the eight W1'
//                     fragments (rt = 2 b + {0, 1}, k-step 4 p + kk).  Per accumulator the MFMA order is pass ascending, then kk = 0..3.
//                     W1' never enters LDS: a fragment (1 KB, fragment-major in w1f, an L2 hit) is loaded by global_load_dwordx4 into this
//                     wave's registers, ONE register set: the successor (same rt, kk of the next pass) is requested right after the
//                     fragment's fourth MFMA of the step (kk outer, tile inner) and has the rest of the step to arrive.  mid1' leaves at a
//                     tile's last pass: bias + ReLU + transpose through the wave's 4 KB buffer, tile by tile, to m1 + row * 256 + 64 b.
// The B-waves are also the loaders, twelve LDS-DMA pieces each per step, issued right after the barrier: W3 of pass s + 1 (32 pieces into
// slot (s + 1) & 1: waves 4, 5 twelve each, waves 6, 7 four each) and, on waves 6 and 7, the shortcut slices of pass s + 2 of two tiles
// each (8 pieces) into stage buffer (s + 2) % 4 -- the buffer whose store-out was read at step s - 1; live buffers are {s - 1, s, s + 1,
// s + 2}.
// vmcnt by hand (only loads in a B-wave's queue, so they retire in order; none of them is visible to the compiler's wait-count pass):
//   queue of a step   [12 DMA pieces: W3 first, then shortcut] [8 W1' fragments, in the order they are consumed]
//   top of a step     W3 of this step must be in LDS before the barrier: vmcnt(8) on waves 4, 5 and vmcnt(16) on waves 6, 7 (the W1'
//                     fragments, and the shortcut pieces behind the four W3 pieces, stay in flight);
//   fragment j        behind it: 7 - j older fragments, this step's 12 pieces, the j successors already requested: vmcnt(19), always.  The
//                     newest DMA pieces stay in flight across it; the shortcut slice of pass s + 1 is forced by the first of these waits
//                     of step s, one step after its request.
//   after mid1' rows  stores retire out of order with loads: the next top-of-step wait is vmcnt(0) (`drain`).
// The loads of the last steps run past the end (W3 / W1' wrap to pass 0, shortcut rows clamp to pixel P - 1, nobody reads them) so that
// the counts hold everywhere; a final vmcnt(0) keeps LDS-DMA from landing after the workgroup has ended.
// In place (x_next over the shortcut operand): every (pixel, 64-channel slice) is loaded (request at step s - 2, in LDS by step s) before
// it is stored (step s + 1), and no other workgroup touches those pixels.
// Same passes, k order per accumulator, rounding points and hence the same bits as the 32-channel-step form it replaces (r25;
// tests/test_gpu_chain256_bits.py) and as the one-role kernel.
// LDS: W3 slots 2 x 32 KB | stage 4 tiles x 4 x 4 KB | mid1' staging 4 x 4 KB | biases 5 KB = 149 KB.
// ---------------------------------------------------------------------------------------------------------------------------
// One W1' fragment into registers, from inline assembly (uniform base + 16 bytes per lane): the compiler's wait-count pass does not see it,
// so it puts no vmcnt(0) in front of the LDS-DMA prefetch.  The destination counts as written at once: every consumer sits behind a
// counted wait that names the registers (chain_wait_frag).  (s_nop 4: the base may come fresh from a v_readfirstlane.)
__device__ __forceinline__ void chain_gld16(bf16x8& d, const void* sbase, unsigned voff) {
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=v"(d) : "v"(voff), "s"(sbase) : "memory");
}
__device__ __forceinline__ void chain_wait_frag(bf16x8& d) { asm volatile("s_waitcnt vmcnt(19)" : "+v"(d) : : "memory"); }

constexpr int kRolesLdsBytes = 2 * 32768 + 4 * 4 * 4096 + 4 * 4096 + (1024 + 256) * 4;      // weights | stage rings | mid1' staging | biases
__global__ __launch_bounds__(512) void chain256_roles_kernel(ChainArgs a) {
  constexpr int MID = 256, COUT = 4 * MID, KS = MID / 16, NP = COUT / 64, NTL = 4, NBUF = 4;
  constexpr int SLOT = 2 * KS * 1024, WBYTES = 2 * SLOT;         // a slot: the 32 W3 fragments of a pass (two row tiles x 16 k-steps)
  constexpr int STG = NBUF * 4096, M1S = WBYTES + NTL * STG, BIAS = M1S + NTL * 4096;
  static_assert(BIAS + (COUT + MID) * 4 == kRolesLdsBytes, "host launch and kernel disagree on the LDS layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31, drow = lane >> 3, dslot = lane & 7;
  const unsigned lds0 = (unsigned)(unsigned long)(las_ptr)smem;
  float* sB3 = (float*)(smem + BIAS);
  float* sB1 = sB3 + COUT;
  for (int i = tid; i < COUT; i += 512) sB3[i] = a.b3[i];
  for (int i = tid; i < MID; i += 512) sB1[i] = a.b1[i];
  const int ntile = (a.P + 31) / 32, nset = (ntile + NTL - 1) / NTL;
  const int n_iter = (nset - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;      // (idle tiles of the last set still take part)
  if (n_iter <= 0) return;
  const int G = n_iter * NP;                                    // steps = passes of this workgroup
  auto tile_p0 = [&](int it, int T) { return (((int)blockIdx.x + it * (int)gridDim.x) * NTL + T) * 32; };     // >= P for idle tiles: loads clamp, stores are masked
  // shortcut slice of global pass Pg for tile T -> stage buffer Pg % NBUF (4 pieces)
  auto issue_x = [&](int T, int Pg) {
    if (a.dbg & 4) return;
    const int p0 = tile_p0(Pg / NP, T), p = Pg % NP;
    unsigned char* sb = smem + WBYTES + T * STG + (Pg % NBUF) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 8 * i + drow;
      const unsigned off = ((unsigned)min(p0 + row, a.P - 1) * COUT + p * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) * 2u;
      chain_glds16((const unsigned char*)a.x + off, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(sb - smem) + i * 1024));
    }
  };
  // W3 of pass g + 1 into slot (g + 1) & 1: B-wave b's share of its 32 pieces (waves 4, 5: twelve each, waves 6, 7: four each)
  auto issue_w3 = [&](int g, int b) {
    if (a.dbg & 2) return;
    const int first = b < 2 ? 12 * b : 16 + 4 * b, n = b < 2 ? 12 : 4;
    const unsigned lb = lds0 + (unsigned)(((g + 1) & 1) * SLOT);
    const unsigned char* src = (const unsigned char*)a.w3f + (unsigned)(((g + 1) % NP) * SLOT) + lane * 16u;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      if (i >= n || ((a.dbg & 1) && (i & 1))) continue;
      chain_glds16(src + (first + i) * 1024, __builtin_amdgcn_readfirstlane(lb + (unsigned)((first + i) * 1024)));
    }
  };
  // prologue: W3 of pass 0, shortcut slices of passes 0 and 1
  if (wave >= 4) issue_w3(-1, wave - 4);
  if (wave >= 6) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) { issue_x(2 * (wave - 6) + tt, 0); }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) { issue_x(2 * (wave - 6) + tt, 1); }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");       // biases in LDS (this also drains the prologue loads once)

  if (wave < 4) {
    // ================================================= A-wave: tile T = wave =================================================
    const int T = wave;
    unsigned char* const stg = smem + WBYTES + T * STG;
    bf16x8 m2f[KS];
    __builtin_amdgcn_s_setprio(2);         // the A-wave's MFMAs go first on the pipe it shares with a B-wave: its epilogue then runs under the B-wave's
#pragma unroll 1
    for (int g = 0; g <= G; ++g) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (this wave's stage writes of the previous step are in LDS)
      if (g < G) {
        const int p = g % NP;
        if (p == 0) {
          const int px = min(tile_p0(g / NP, T) + l31, a.P - 1);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) m2f[ks] = *(const bf16x8*)(a.m2 + (long)px * MID + 16 * ks + 8 * half);
          __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0) HERE, once per tile, as a real instruction the compiler's wait-count pass sees: left to it (or
                                                   // hidden in an asm statement) counted vmcnt waits land on the main path of every step and drain the stores
        }
        const uint4* w3 = (const uint4*)(smem + (g & 1) * SLOT);
        unsigned char* sb = stg + (g % NBUF) * 4096;
        uint2 xv[2][4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) xv[ct][gq] = *(const uint2*)(sb + l31 * 128 + (((ct * 4 + gq) ^ ((l31 >> 1) & 7)) << 4) + 8 * half);
        // two independent chains of sixteen MFMAs (rows [64 p, +32) and [64 p + 32, +32)), interleaved.  The 32 weight fragments come in four
        // batches (4 k-steps x 2 chains) through two register sets, a batch requested two batches ahead of its MFMAs: left to itself the
        // scheduler reads two fragments at a time and waits for LDS between every two MFMAs.
        f32x16 ac[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) ac[ct][r] = 0.f;
        bf16x8 wf[2][8];
        auto read_w3 = [&](int set, int bt) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) wf[set][2 * i + ct] = *(const bf16x8*)&w3[(ct * KS + 4 * bt + i) * 64 + lane];
        };
        read_w3(0, 0);
        read_w3(1, 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) ac[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[bt & 1][2 * i + ct], m2f[4 * bt + i], ac[ct], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (bt + 2 < 4) {
            read_w3(bt & 1, bt + 2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            uint2* sp = (uint2*)(sb + l31 * 128 + (((ct * 4 + gq) ^ ((l31 >> 1) & 7)) << 4) + 8 * half);
            const float4 bv = *(const float4*)(sB3 + p * 64 + ct * 32 + 8 * gq + 4 * half);
            const uint2 x2 = xv[ct][gq];
            const float v0 = fmaxf(ac[ct][4 * gq + 0] + bv.x + bf2f(x2.x & 0xffff), 0.f), v1 = fmaxf(ac[ct][4 * gq + 1] + bv.y + bf2f(x2.x >> 16), 0.f);
            const float v2 = fmaxf(ac[ct][4 * gq + 2] + bv.z + bf2f(x2.y & 0xffff), 0.f), v3 = fmaxf(ac[ct][4 * gq + 3] + bv.w + bf2f(x2.y >> 16), 0.f);
            *sp = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
          }
      }
      if (g >= 1) {
        // the slice of pass g - 1 is complete (this wave, step g - 1, fenced by the barrier above): out, 16-byte coalesced rows
        const int Pf = g - 1, p0 = tile_p0(Pf / NP, T), p = Pf % NP;
        const unsigned char* sb = stg + (Pf % NBUF) * 4096 + lane * 16;
        const uint4 v0 = *(const uint4*)sb, v1 = *(const uint4*)(sb + 1024), v2 = *(const uint4*)(sb + 2048), v3 = *(const uint4*)(sb + 3072);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        auto put = [&](int i, const uint4& v) {
          const int row = 8 * i + drow;
          if (p0 + row < a.P && !(a.dbg & 8)) *(uint4*)((unsigned char*)a.xn + ((unsigned)(p0 + row) * COUT + p * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) * 2u) = v;
        };
        put(0, v0); put(1, v1); put(2, v2); put(3, v3);
      }
    }
  } else {
    // ================================================= B-wave b = wave - 4: mid1' channels [64 b, +64) of the four tiles =========
    const int b = wave - 4;
    unsigned char* const m1s = smem + M1S + b * 4096;
    const unsigned lrd = (unsigned)(l31 * 128 + 8 * half) | (unsigned)(((l31 >> 1) & 7) << 4);      // stage read: chunk c of this lane's row at lrd ^ (c << 4)
    const unsigned voff = lane * 16u;
    f32x16 m1acc[NTL][2];
#pragma unroll
    for (int T = 0; T < NTL; ++T)
#pragma unroll
      for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
        for (int r = 0; r < 16; ++r) m1acc[T][r2][r] = 0.f;
    bf16x8 wf[8];                            // W1' fragments of the pass in hand, j = 2 kk + r2: (rt = 2 b + r2, k-step 4 p + kk)
#pragma unroll
    for (int j = 0; j < 8; ++j) wf[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    auto load_w1 = [&](int j, int pass) {
      if ((a.dbg & 2) || ((a.dbg & 1) && (j & 1))) return;
      chain_gld16(wf[j], (const unsigned char*)a.w1f + (unsigned)((((2 * b + (j & 1)) * (COUT / 16)) + 4 * pass + (j >> 1)) * 1024), voff);
    };
    bool drain = false;                      // this wave has stores in its queue (mid1' rows): the next counted wait must be a full one
    // step 0 (nothing to consume yet) stands outside the loop: the same queue as every step, the fragments of pass 0 in the place of the
    // successors.  (As a branch of the loop body it made the register allocator copy and spill the accumulators around every MFMA.)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    issue_w3(0, b);
    if (wave >= 6) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) issue_x(2 * (wave - 6) + tt, 2);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) load_w1(j, 0);
#pragma unroll 1
    for (int g = 1; g <= G; ++g) {
      // W3 of pass g (requested at step g - 1, ahead of the W1' fragments and, on waves 6 and 7, of eight shortcut pieces) has landed
      if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (wave < 6) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      drain = false;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      const int q = g - 1, p = q % NP, pn = g % NP;            // the pass the A-waves finished before this barrier; the pass after it
      const unsigned char* sb = smem + WBYTES + (q % NBUF) * 4096;
      // x_next fragments of the four tiles, 16 channels (kk) at a time: the halves of kk + 1 are requested before the MFMAs of kk and
      // joined after them (the counted lgkmcnt waits are the compiler's)
      uint2 xr[NTL][2];
      bf16x8 xf[NTL];
      unsigned tb[NTL];                                        // tile bases the compiler cannot relate: it would pair the reads of two tiles
#pragma unroll                                                 // (ds_read2st64) and move every half into place behind a full wait, ahead of the MFMAs
      for (int T = 0; T < NTL; ++T) { tb[T] = (unsigned)(T * STG); asm volatile("" : "+v"(tb[T])); }
      auto read_x = [&](int kk) {
#pragma unroll
        for (int T = 0; T < NTL; ++T) {
          xr[T][0] = *(const uint2*)(sb + tb[T] + (lrd ^ (unsigned)((2 * kk) << 4)));
          xr[T][1] = *(const uint2*)(sb + tb[T] + (lrd ^ (unsigned)((2 * kk + 1) << 4)));
        }
      };
      auto join_x = [&]() {
#pragma unroll
        for (int T = 0; T < NTL; ++T) { *(uint2*)&xf[T] = xr[T][0]; *((uint2*)&xf[T] + 1) = xr[T][1]; }
      };
      read_x(0);                                               // (ahead of the DMA issue: it arrives behind it)
      __builtin_amdgcn_sched_barrier(0);
      issue_w3(g, b);
      if (wave >= 6) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) issue_x(2 * (wave - 6) + tt, g + 2);
      }
      join_x();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        __builtin_amdgcn_sched_barrier(0);
        if (kk + 1 < 4) {
          read_x(kk + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2) {
          const int j = 2 * kk + r2;
          chain_wait_frag(wf[j]);
#pragma unroll
          for (int T = 0; T < NTL; ++T) m1acc[T][r2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], xf[T], m1acc[T][r2], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);                   // (the four MFMAs have issued: the registers may be requested again)
          load_w1(j, pn);
        }
        if (kk + 1 < 4) join_x();
      }
      if (p == NP - 1) {
        // mid1' = relu(. + b1) of the four tiles that just ended, one tile (32 px x this wave's 64 channels) at a time through the staging buffer
#pragma unroll
        for (int T = 0; T < NTL; ++T) {
          const int p0 = tile_p0(q / NP, T);
#pragma unroll
          for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const float4 bv = *(const float4*)(sB1 + (2 * b + r2) * 32 + 8 * gq + 4 * half);
              const float v0 = fmaxf(m1acc[T][r2][4 * gq + 0] + bv.x, 0.f), v1 = fmaxf(m1acc[T][r2][4 * gq + 1] + bv.y, 0.f);
              const float v2 = fmaxf(m1acc[T][r2][4 * gq + 2] + bv.z, 0.f), v3 = fmaxf(m1acc[T][r2][4 * gq + 3] + bv.w, 0.f);
              *(uint2*)(m1s + l31 * 128 + (((r2 * 4 + gq) ^ ((l31 >> 1) & 7)) << 4) + 8 * half) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
            }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_wave_barrier();
          const unsigned char* sl = m1s + lane * 16;
          const uint4 v0 = *(const uint4*)sl, v1 = *(const uint4*)(sl + 1024), v2 = *(const uint4*)(sl + 2048), v3 = *(const uint4*)(sl + 3072);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_wave_barrier();
          auto put = [&](int i, const uint4& v) {
            const int row = 8 * i + drow;
            if (p0 + row < a.P && !(a.dbg & 8)) *(uint4*)(a.m1 + (long)(p0 + row) * MID + b * 64 + ((dslot ^ ((row >> 1) & 7)) << 3)) = v;
          };
          put(0, v0); put(1, v1); put(2, v2); put(3, v3);
#pragma unroll
          for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
            for (int r = 0; r < 16; ++r) m1acc[T][r2][r] = 0.f;
        }
        drain = true;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // no LDS-DMA piece may land after the workgroup has ended
  }
}

}  // namespace relnet

using namespace relnet;

// x_next = relu(conv1x1(mid2; W3, b3) + x), mid1_next = relu(conv1x1(x_next; W1n, b1n)) over P pixels (NHWC bf16, dense
// rows).  mid = 64 (res2: 64 -> 256 -> 64) or 128 (res3: 128 -> 512 -> 128).  w3f = relnet_pack_w_frag of W3 [4 mid][mid]; w1f = W1n [mid][4 mid] in the
// accumulator-permuted fragment order (ops.pack_chain_w1).  Replaces two relnet_conv2d_nhwc launches
// (resnet_v1_101_rcnn_base.py: res<s><u>_branch2c + shortcut + relu, res<s><u+1>_branch2a + relu).
static int g_chain_dbg = 0;        // timing ablations of chain256_roles_kernel (ChainArgs::dbg): results are wrong while it is non-zero
extern "C" void relnet_chain_debug(int flags) { g_chain_dbg = flags; }

extern "C" int relnet_bottleneck_chain(const void* mid2, const void* x, const void* w3f, const void* w1f, const float* b3,
                                       const float* b1, void* x_next, void* mid1_next, long P, int mid, void* stream) {
  RELNET_REQUIRE(mid2 && x && w3f && b3 && x_next, "relnet_bottleneck_chain: null operand");
  RELNET_REQUIRE((w1f && b1 && mid1_next) || (!w1f && !b1 && !mid1_next), "relnet_bottleneck_chain: w1f, b1 and mid1_next are given together (or all NULL: expand + shortcut + ReLU only)");
  RELNET_REQUIRE(mid == 64 || mid == 128 || mid == 256 || (mid == 512 && !mid1_next), "relnet_bottleneck_chain: mid = %d unsupported (64, 128, 256; 512 without the reduce product)", mid);
  RELNET_REQUIRE(P > 0 && P * 8 * mid < (1L << 32), "relnet_bottleneck_chain: bad pixel count %ld (the 4 mid-channel map must stay below 4 GiB)", P);
  ChainArgs a;
  a.m2 = (const unsigned short*)mid2; a.x = (const unsigned short*)x; a.w3f = (const uint4*)w3f; a.w1f = (const uint4*)w1f;
  a.b3 = b3; a.b1 = b1; a.xn = (unsigned short*)x_next; a.m1 = (unsigned short*)mid1_next; a.P = (int)P;
  a.xin = nullptr; a.wpf = nullptr; a.dbg = g_chain_dbg;
  a.H = a.W = a.Ho = a.Wo = 0;
  static relnet::PerDeviceOnce attr_once;
  if (attr_once.first()) {
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<64, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<128, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<64, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<128, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<256, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<512, true, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)chain256_roles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  const long ntile = (P + 31) / 32;
  const unsigned grid = (unsigned)(ntile < 8 * 256 ? (ntile + 7) / 8 : 256);     // persistent: one workgroup per CU
  const size_t lds = 65536 /* weights: resident (mid 64) or two ring slots (mid 128) */ + 65536 /* 8 x 2 stage buffers */ + (size_t)5 * mid * 4;
  if (mid1_next) {
    if (mid == 64) bottleneck_chain_kernel<64, false><<<grid, 512, lds, (hipStream_t)stream>>>(a);
    else if (mid == 128) bottleneck_chain_kernel<128, true><<<grid, 512, lds, (hipStream_t)stream>>>(a);
    else {
      const long nset = (ntile + 3) / 4;
      chain256_roles_kernel<<<(unsigned)(nset < 256 ? nset : 256), 512, relnet::kRolesLdsBytes, (hipStream_t)stream>>>(a);
    }
  } else {
    if (mid == 64) bottleneck_chain_kernel<64, false, false><<<grid, 512, lds, (hipStream_t)stream>>>(a);
    else if (mid == 128) bottleneck_chain_kernel<128, true, false><<<grid, 512, lds, (hipStream_t)stream>>>(a);
    else if (mid == 256) bottleneck_chain_kernel<256, true, false><<<grid, 512, lds, (hipStream_t)stream>>>(a);
    else bottleneck_chain_kernel<512, true, false, 2><<<grid, 512, lds, (hipStream_t)stream>>>(a);
  }
  return check_launch("relnet_bottleneck_chain");
}

// Last unit of a stage whose successor subsamples by two (res2c, res3b3 of the non-FPN trunk): x_next = relu(conv1x1(mid2; W3, b3) + x)
// at the even (y, x) pixels only.  mid2 [B][Ho][Wo][mid] and x_next [B][Ho][Wo][4 mid] are compact (Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1),
// the shortcut x [B][H][W][4 mid] is the full map (all dense NHWC bf16); x_next must not alias x.  mid = 64 or 128.  Same bits as
// relnet_bottleneck_chain (w1f = NULL) at those pixels.
extern "C" int relnet_bottleneck_chain_s2(const void* mid2, const void* x, const void* w3f, const float* b3, void* x_next, int B,
                                          int H, int W, int mid, void* stream) {
  RELNET_REQUIRE(mid2 && x && w3f && b3 && x_next && x_next != x, "relnet_bottleneck_chain_s2: null operand (or x_next == x: this form is never in place)");
  RELNET_REQUIRE(mid == 64 || mid == 128, "relnet_bottleneck_chain_s2: mid = %d unsupported (64, 128)", mid);
  RELNET_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W * 8 * mid < (1L << 32),
                 "relnet_bottleneck_chain_s2: bad geometry B=%d H=%d W=%d (the full 4 mid-channel map must stay below 4 GiB)", B, H, W);
  ChainArgs a;
  a.m2 = (const unsigned short*)mid2; a.x = (const unsigned short*)x; a.w3f = (const uint4*)w3f; a.w1f = nullptr;
  a.b3 = b3; a.b1 = nullptr; a.xn = (unsigned short*)x_next; a.m1 = nullptr;
  a.xin = nullptr; a.wpf = nullptr; a.dbg = 0;
  a.H = H; a.W = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
  const long P = (long)B * a.Ho * a.Wo;
  a.P = (int)P;
  static relnet::PerDeviceOnce attr_once;
  if (attr_once.first()) {
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<64, false, false, 1, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<128, true, false, 1, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  const long ntile = (P + 31) / 32;
  const unsigned grid = (unsigned)(ntile < 8 * 256 ? (ntile + 7) / 8 : 256);
  const size_t lds = 65536 + 65536 + (size_t)5 * mid * 4;       // as relnet_bottleneck_chain
  if (mid == 64) bottleneck_chain_kernel<64, false, false, 1, false, true><<<grid, 512, lds, (hipStream_t)stream>>>(a);
  else bottleneck_chain_kernel<128, true, false, 1, false, true><<<grid, 512, lds, (hipStream_t)stream>>>(a);
  return check_launch("relnet_bottleneck_chain_s2");
}

// First unit of res2 (projection shortcut, stride 1): x_next = relu(conv1x1(mid2; W3) + conv1x1(x_in; Wp) + b3p), b3p = b3 + bp, and
// (optionally) mid1_next = relu(conv1x1(x_next; W1n, b1n)) in one kernel: the branch1 convolution of the reference graph
// (resnet_v1_101_rcnn_base.py: res2a_branch1 + bn2a_branch1) becomes four more k-steps of the expand product.  mid = 64 only;
// w3f / wpf = relnet_pack_w_frag of W3 / Wp [256][64]; x_in [P][64] dense bf16.
extern "C" int relnet_bottleneck_chain_proj(const void* mid2, const void* x_in, const void* w3f, const void* wpf, const void* w1f,
                                            const float* b3p, const float* b1, void* x_next, void* mid1_next, long P, int mid,
                                            void* stream) {
  RELNET_REQUIRE(mid2 && x_in && w3f && wpf && b3p && x_next, "relnet_bottleneck_chain_proj: null operand");
  RELNET_REQUIRE((w1f && b1 && mid1_next) || (!w1f && !b1 && !mid1_next), "relnet_bottleneck_chain_proj: w1f, b1 and mid1_next are given together (or all NULL)");
  RELNET_REQUIRE(mid == 64, "relnet_bottleneck_chain_proj: mid = %d unsupported (64)", mid);
  RELNET_REQUIRE(P > 0 && P * 8 * mid < (1L << 32), "relnet_bottleneck_chain_proj: bad pixel count %ld (x_next is addressed with 32-bit byte offsets: the 4 mid-channel map must stay below 4 GiB)", P);
  ChainArgs a;
  a.m2 = (const unsigned short*)mid2; a.x = nullptr; a.w3f = (const uint4*)w3f; a.w1f = (const uint4*)w1f;
  a.b3 = b3p; a.b1 = b1; a.xn = (unsigned short*)x_next; a.m1 = (unsigned short*)mid1_next; a.P = (int)P;
  a.xin = (const unsigned short*)x_in; a.wpf = (const uint4*)wpf; a.dbg = 0;
  a.H = a.W = a.Ho = a.Wo = 0;
  static relnet::PerDeviceOnce attr_once;
  if (attr_once.first()) {
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<64, false, true, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)bottleneck_chain_kernel<64, false, false, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  const long ntile = (P + 31) / 32;
  const unsigned grid = (unsigned)(ntile < 8 * 256 ? (ntile + 7) / 8 : 256);
  const size_t lds = (size_t)4 * (8192 + 8192 + (mid1_next ? 8192 : 0)) + 8 * 4096 + (size_t)5 * mid * 4;
  if (mid1_next) bottleneck_chain_kernel<64, false, true, 1, true><<<grid, 512, lds, (hipStream_t)stream>>>(a);
  else bottleneck_chain_kernel<64, false, false, 1, true><<<grid, 512, lds, (hipStream_t)stream>>>(a);
  return check_launch("relnet_bottleneck_chain_proj");
}

// ---------------------------------------------------------------------------------------
// 3x3 convolution of the 64-channel bottleneck (res2*_branch2b: stride 1, pad 1, BN folded, ReLU) with the input tile
// and its halo resident in LDS.  The implicit-GEMM kernel fills LDS once per tap (9 x the input through L2 -> LDS,
// 2.3 GB per launch at B = 54, the measured bound of its 297 us); here a (8+2) x (32+2)-pixel halo tile is fetched ONCE
// (1.33 x the input) and the nine taps are row offsets into it.
// Workgroup = 8 x 32 output pixels, persistent over tiles with the next halo tile in flight; wave (c, r) owns output
// channels 32 c .. 32 c + 31 for pixel rows 2 r, 2 r + 1.  Its 36 weight fragments (32 channels x 576) stay in VGPRs for
// the life of the workgroup, so LDS serves only the pixel operand.
// S2 (the stride-2 output form: res2c_branch2b when only the even pixels of res2c are read): out[b][yo][xo] = the dense result at
// (2 yo, 2 xo), from the same 36 k-steps in the same order.  Workgroup = 4 x 32 output pixels (one row per wave: a single MFMA
// chain), whose halo is 9 rows x 65 columns.  A row is stored de-interleaved -- its 33 even columns, then its 32 odd ones -- so that
// the 32 lanes of a tap still read 32 CONSECUTIVE pixel slots (columns 2 l + dx at stride 2 would leave half the banks idle), rows of 65
// slots back to back: 585 slots, 74 DMA instructions, 74 KiB per buffer.  Two of them leave no room for the output staging, which
// therefore reuses the halo buffer the tile has just finished reading (one more workgroup barrier per tile).
// ---------------------------------------------------------------------------------------
namespace relnet {

__device__ __attribute__((aligned(16))) const unsigned int g_zero_chunk[4] = {0u, 0u, 0u, 0u};

struct Halo3Args {
  const unsigned short* in;    // [B][H][W][64] bf16, dense
  const uint4* wf;             // W [64][576] (k = tap * 64 + c) in fragment order (relnet_pack_w_frag)
  const float* bias;           // [64]
  unsigned short* out;         // [B][H][W][64]
  int B, H, W, relu;
  int tiles_x, tiles_y;        // ceil(W / 32), ceil(H / 8)  (S2: ceil(Wo / 32), ceil(Ho / 4))
  int Ho, Wo;                  // output map (S2: (H - 1) / 2 + 1, (W - 1) / 2 + 1; otherwise H, W)
};

constexpr int kHaloW = 34, kHaloSlots = 40;                 // halo columns used / allocated per row (5 x 8 pixels)
constexpr int kHaloBytes = 10 * kHaloSlots * 128;           // 50 DMA instructions x 1 KiB
constexpr int kHalo2Row = 65, kHalo2Even = 33;              // S2: slots per halo row (33 even columns | 32 odd columns)
constexpr int kHalo2Dma = (9 * kHalo2Row + 7) / 8;          // 74 DMA instructions x 1 KiB
constexpr int kHalo2Bytes = kHalo2Dma * 1024;

template <bool S2>
__global__ __launch_bounds__(512) void conv3x3_c64_halo_kernel(Halo3Args a) {
  constexpr int NR = S2 ? 1 : 2;                             // output rows per wave; the tile is 4 NR rows x 32 columns
  constexpr int HB = S2 ? kHalo2Bytes : kHaloBytes;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sOutDense = smem + 2 * HB;                  // [256 px][128 B], chunk c of pixel p at slot c ^ ((p >> 1) & 7)  (S2: the halo buffer just read)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keeps tile / row arithmetic on the scalar unit
  const int half = lane >> 5, l31 = lane & 31;
  const int chh = wave & 1, rg = wave >> 1;                  // channel half, row group
  bf16x8 wfrag[36];
#pragma unroll
  for (int ks = 0; ks < 36; ++ks) wfrag[ks] = *(const bf16x8*)&a.wf[(chh * 36 + ks) * 64 + lane];
  float* sBias = (float*)(smem + 2 * HB + (S2 ? 0 : 32768));   // [64]
  if (tid < 64) sBias[tid] = a.bias[tid];
  const int per_img = a.tiles_x * a.tiles_y;
  const int ntile = a.B * per_img;

  // halo tile in LDS: [10 rows][40 pixel slots][128 B] (34 used per row; 5 one-KiB DMA instructions per row), chunk c of
  // slot q at position c ^ ((q >> 1) & 7), q = row * 40 + column.  Everything per-instruction is wave-uniform (scalar)
  // except (lane >> 3, lane & 7): no per-lane address state survives between tiles (spilled addresses would be reloaded
  // through scratch, whose vmcnt wait would serialise the LDS-direct loads behind each other -- measured 9 us per tile).
  auto issue_halo = [&](int t, unsigned char* buf) {
    asm volatile("" : "+s"(t));                             // opaque: no loop-carried (and then spilled) per-lane pointers
    const int b = t / per_img, ty = (t % per_img) / a.tiles_x, tx = t % a.tiles_x;
    const int y0 = ty * 8 - 1, x0 = tx * 32 - 1;
    const unsigned short* img = a.in + (long)b * a.H * a.W * 64;
    int ln = lane;
    asm volatile("" : "+v"(ln));                            // opaque too: the per-lane parts are recomputed per tile, not kept live
    const int r8 = ln >> 3, slot = ln & 7;
    if constexpr (S2) {
      const int ys = 8 * ty - 1, xs = 64 * tx - 1;           // input pixel of halo (row 0, column 0)
#pragma unroll
      for (int i = 0; i < (kHalo2Dma + 7) / 8; ++i) {
        const int j = wave + 8 * i;                          // DMA instruction j: slots 8 j .. 8 j + 7 of the linear [9][65] slot order
        if (j >= kHalo2Dma) break;
        const int q = 8 * j + r8, hy = q / kHalo2Row, sl = q - kHalo2Row * hy;
        const int hx = sl < kHalo2Even ? 2 * sl : 2 * (sl - kHalo2Even) + 1;
        const int y = ys + hy, x = xs + hx;
        const int sw = (4 * j + (r8 >> 1)) & 7;              // (q >> 1) & 7
        const bool ok = hy < 9 && y >= 0 && y < a.H && x >= 0 && x < a.W;
        const void* src = ok ? (const void*)(img + ((long)y * a.W + x) * 64 + ((slot ^ sw) << 3)) : (const void*)g_zero_chunk;
        __builtin_amdgcn_global_load_lds((gas_ptr)src, (las_ptr)(buf + j * 1024), 16, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int j = wave + 8 * i;                            // DMA instruction j: halo row j / 5, pixel slots 8 (j % 5) ..
      if (j >= 50) break;
      const int hy = j / 5, part = j - 5 * hy;
      const int y = y0 + hy, hx = part * 8 + r8, x = x0 + hx;
      const int sw = (4 * (hy + part) + (r8 >> 1)) & 7;      // ((hy * 40 + hx) >> 1) & 7
      const bool ok = hx < kHaloW && y >= 0 && y < a.H && x >= 0 && x < a.W;
      const void* src = ok ? (const void*)(img + ((long)y * a.W + x) * 64 + ((slot ^ sw) << 3)) : (const void*)g_zero_chunk;
      __builtin_amdgcn_global_load_lds((gas_ptr)src, (las_ptr)(buf + j * 1024), 16, 0, 0);
    }
  };

  int t = blockIdx.x;
  if (t < ntile) issue_halo(t, smem);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  int cur = 0;
  for (; t < ntile; t += gridDim.x, cur ^= 1) {
    // the next tile's halo is requested first and is only waited for after this tile's arithmetic; this tile's stores are
    // issued after that wait and drain during the NEXT tile's arithmetic (loads and stores share vmcnt and complete out of
    // order with respect to each other, so the only safe wait is vmcnt(0): it is placed where both have had a tile's time)
    const int tn = t + gridDim.x;
    if (tn < ntile) issue_halo(tn, smem + (cur ^ 1) * HB);
    const unsigned char* hb = smem + cur * HB;
    unsigned char* sOut = S2 ? smem + cur * HB : sOutDense;
    int lq = l31;
    asm volatile("" : "+v"(lq));                            // the 72 swizzled read offsets are recomputed per tile, not held in VGPRs
    f32x16 acc[NR];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rr][r] = 0.f;
    {
      // 36 k-steps (tap, 16-channel block); the two pixel rows alternate (two independent MFMA chains) and the fragments
      // of step s + 2 are requested before the MFMAs of step s
      auto frag = [&](int s_, int rr) -> bf16x8 {
        const int tap = s_ >> 2, kb = s_ & 3, dy = tap / 3, dx = tap % 3;
        const int hp = S2 ? (2 * rg + dy) * kHalo2Row + lq + (dx == 1 ? kHalo2Even : dx >> 1)      // column 2 l + dx of row 2 rg + dy
                          : (2 * rg + rr + dy) * kHaloSlots + lq + dx;
        return *(const bf16x8*)(hb + hp * 128 + (((2 * kb + half) ^ ((hp >> 1) & 7)) << 4));
      };
      bf16x8 pq[3][NR];
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) { pq[0][rr] = frag(0, rr); pq[1][rr] = frag(1, rr); }
#pragma unroll
      for (int s_ = 0; s_ < 36; ++s_) {
        if (s_ + 2 < 36) {
#pragma unroll
          for (int rr = 0; rr < NR; ++rr) pq[(s_ + 2) % 3][rr] = frag(s_ + 2, rr);
        }
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) acc[rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag[s_], pq[s_ % 3][rr], acc[rr], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (S2) __builtin_amdgcn_s_barrier();         // every wave has read this halo: it becomes the output staging
    // bias -> ReLU -> bf16 -> staging [pixel][64 channels]
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
      const int p = (NR * rg + rr) * 32 + l31;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bq = *(const float4*)(sBias + chh * 32 + 8 * g + 4 * half);
        float v[4] = {acc[rr][4 * g] + bq.x, acc[rr][4 * g + 1] + bq.y, acc[rr][4 * g + 2] + bq.z, acc[rr][4 * g + 3] + bq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a.relu ? fmaxf(v[e], 0.f) : v[e];
        *(uint2*)(sOut + p * 128 + (((chh * 4 + g) ^ ((p >> 1) & 7)) << 4) + 8 * half) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // both channel halves of every pixel are staged
    {
      const int b = t / per_img, ty = (t % per_img) / a.tiles_x, tx = t % a.tiles_x;
      unsigned short* img = a.out + (long)b * a.Ho * a.Wo * 64;
      const unsigned char* so = sOut + wave * (2048 * NR) + lane * 16;
      const uint4 v0 = *(const uint4*)so, v1 = *(const uint4*)(so + 1024);
      uint4 v2 = v0, v3 = v1;
      if constexpr (NR == 2) { v2 = *(const uint4*)(so + 2048); v3 = *(const uint4*)(so + 3072); }
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // next halo landed (this wave's part); staging read
      auto put = [&](int i, const uint4& v) {
        const int p = 8 * (wave * 2 * NR + i) + (lane >> 3), slot = lane & 7;
        const int y = ty * 4 * NR + (p >> 5), x = tx * 32 + (p & 31);
        if (y < a.Ho && x < a.Wo) *(uint4*)(img + ((long)y * a.Wo + x) * 64 + ((slot ^ ((p >> 1) & 7)) << 3)) = v;
      };
      put(0, v0); put(1, v1);
      if constexpr (NR == 2) { put(2, v2); put(3, v3); }
    }
    __builtin_amdgcn_s_barrier();                           // every wave's part of the next halo is in LDS; staging is free
  }
}

}  // namespace relnet

// 3x3 / stride 1 / pad 1 convolution + bias (+ ReLU) of a dense 64-channel NHWC bf16 tensor (res2*_branch2b with BN folded;
// resnet_v1_101_rcnn_base.py:52-56).  w_frag = relnet_pack_w_frag of the packed weight [64][9 * 64] (k = (r * 3 + s) * 64 + c).
extern "C" int relnet_conv3x3_c64(const void* in, const void* w_frag, const float* bias, int relu, void* out, int B, int H,
                                  int W, void* stream) {
  RELNET_REQUIRE(in && w_frag && bias && out, "relnet_conv3x3_c64: null operand");
  RELNET_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "relnet_conv3x3_c64: bad geometry B=%d H=%d W=%d", B, H, W);
  Halo3Args a;
  a.in = (const unsigned short*)in; a.wf = (const uint4*)w_frag; a.bias = bias; a.out = (unsigned short*)out;
  a.B = B; a.H = H; a.W = W; a.relu = relu;
  a.tiles_x = (W + 31) / 32; a.tiles_y = (H + 7) / 8; a.Ho = H; a.Wo = W;
  static relnet::PerDeviceOnce attr_once;
  if (attr_once.first()) {
    hipFuncSetAttribute((const void*)conv3x3_c64_halo_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  const long ntile = (long)B * a.tiles_x * a.tiles_y;
  const unsigned grid = (unsigned)(ntile < 256 ? ntile : 256);
  conv3x3_c64_halo_kernel<false><<<grid, 512, 2 * kHaloBytes + 32768 + 256, (hipStream_t)stream>>>(a);
  return check_launch("relnet_conv3x3_c64");
}

// The same convolution at stride 2: out [B][Ho][Wo][64], Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, out[b][yo][xo] = the stride-1 result at
// (2 yo, 2 xo), bit for bit (same k-steps, same order).  Operands as relnet_conv3x3_c64.
extern "C" int relnet_conv3x3_c64_s2(const void* in, const void* w_frag, const float* bias, int relu, void* out, int B, int H,
                                     int W, void* stream) {
  RELNET_REQUIRE(in && w_frag && bias && out, "relnet_conv3x3_c64_s2: null operand");
  RELNET_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "relnet_conv3x3_c64_s2: bad geometry B=%d H=%d W=%d", B, H, W);
  Halo3Args a;
  a.in = (const unsigned short*)in; a.wf = (const uint4*)w_frag; a.bias = bias; a.out = (unsigned short*)out;
  a.B = B; a.H = H; a.W = W; a.relu = relu;
  a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
  a.tiles_x = (a.Wo + 31) / 32; a.tiles_y = (a.Ho + 3) / 4;
  static relnet::PerDeviceOnce attr_once;
  if (attr_once.first()) {
    hipFuncSetAttribute((const void*)conv3x3_c64_halo_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  const long ntile = (long)B * a.tiles_x * a.tiles_y;
  const unsigned grid = (unsigned)(ntile < 256 ? ntile : 256);
  conv3x3_c64_halo_kernel<true><<<grid, 512, 2 * kHalo2Bytes + 256, (hipStream_t)stream>>>(a);
  return check_launch("relnet_conv3x3_c64_s2");
}

// (Measured and dropped: the same halo-resident form for the 256-channel res4 3x3 layers -- halo tile per 64- or 128-channel
//  part, weights [256][64] through a 2-, 3- or 4-slot LDS ring -- reaches 178-186 us against 166 us of the implicit-GEMM ring
//  kernel in isolation.  With 8 fragment MFMAs per 6 LDS fragment reads and a workgroup barrier per weight slab the LDS-read +
//  MFMA rate, not the L2 -> LDS fill it removes, is what bounds those layers.)
