// Guard of the optimizer step, evaluated on the device (train.GradGuard): nothing else stands between a bad gradient and the fp32
// master weights, and the training loop never synchronises, so the host cannot look.
//
//  * relnet_grad_stats          sum of squares (double) and number of non-finite elements (int64) of up to 16 float ranges in ONE launch.
//                               Every workgroup writes its two partials to its OWN slot of a caller-owned workspace; nothing is
//                               accumulated across workgroups here, so there is no atomic of any kind and no counter to reset.
//  * relnet_grad_guard_decide   one workgroup folds the slots of ALL statistics launches of the step (a fixed order: thread t adds slots
//                               t, t + 256, ..., then the fixed shuffle tree, then the waves in wave order) and writes the guard state:
//                               skip, the global-norm clipping scale, the last norm / count, the running totals.  Ordered after the
//                               statistics launches by the stream -- two kernels, not a last-arriver protocol.
//  * relnet_sgd_update_guarded  sgd_update_kernel of train_ops.hip + the state: nothing is written on skip, otherwise the gradient term is
//                               clip((rescale * grad) * scale, +-c) (mx.optimizer.SGD's clip_gradient; off for c < 0).
//
// The grid of a statistics launch is a function of the element counts alone and a thread's elements are a function of the grid, so the
// same input gives the same bits on every run.  A non-finite element (exponent bits all ones) adds to the count and nothing to the sum;
// denormals are finite.  Squares of float32 values are exact in double and cannot overflow it (|x| < 2^128 -> x^2 < 2^256).
#include "common.h"
#include "wave.h"

namespace relnet {

constexpr int kGuardThreads = 256;
constexpr int kGuardWaves = kGuardThreads / kWave;
constexpr int kGuardMaxRanges = 16;                      // ranges per statistics launch (the table travels in the kernel argument)
constexpr long kGuardVecsPerThread = 4;                  // four 16-byte loads per thread before a range's grid grows
constexpr long kGuardElemsPerBlock = kGuardThreads * 4 * kGuardVecsPerThread;       // 4096
constexpr long kGuardMaxBlocksPerRange = 2048;           // grid cap per range: 8 workgroups per CU on 256 CUs, grid-stride beyond

struct GuardSlot { double sumsq; long long nonfinite; };  // one per workgroup of a statistics launch (16 bytes)

struct GuardState {                                       // mirrors relnet_grad_guard_state (include/relnet_hip.h)
  int skip; float scale;
  double last_norm;
  long long last_nonfinite;
  long long steps, skipped, clipped;
  double norm_sum, norm_max;
};
static_assert(sizeof(GuardState) == 64, "relnet_grad_guard_state is 64 bytes");

struct StatsRange { const float* p; long n; int blk_start, blocks; };
struct StatsGroup { StatsRange r[kGuardMaxRanges]; int n; GuardSlot* slots; };

__device__ __forceinline__ void guard_one(float x, double& a, long long& c) {
  const bool bad = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;      // inf or NaN
  const double d = (double)x;
  a += bad ? 0.0 : d * d;
  c += bad ? 1 : 0;
}

static long guard_range_blocks(long n) {
  const long b = (n + kGuardElemsPerBlock - 1) / kGuardElemsPerBlock;
  return b < 1 ? 1 : (b > kGuardMaxBlocksPerRange ? kGuardMaxBlocksPerRange : b);
}

// A range = scalar head up to the first 16-byte boundary (<= 3 elements), 16-byte loads over the aligned body, scalar tail (<= 3).
__global__ __launch_bounds__(kGuardThreads) void grad_stats_kernel(StatsGroup g) {
  __shared__ double s_d[kGuardWaves];
  __shared__ long long s_c[kGuardWaves];
  int ri = 0;
  for (int i = 1; i < g.n; ++i) if ((int)blockIdx.x >= g.r[i].blk_start) ri = i;
  const StatsRange& a = g.r[ri];
  const long rel = (long)blockIdx.x - a.blk_start;
  long head = (long)(((16 - ((uintptr_t)a.p & 15)) & 15) >> 2);
  head = head < a.n ? head : a.n;
  const long nvec = (a.n - head) >> 2, tail = a.n - head - 4 * nvec;
  const float4* body = (const float4*)(a.p + head);
  double acc = 0.0;
  long long cnt = 0;
#pragma unroll 4
  for (long v = rel * kGuardThreads + threadIdx.x; v < nvec; v += (long)a.blocks * kGuardThreads) {
    const float4 x = body[v];
    guard_one(x.x, acc, cnt); guard_one(x.y, acc, cnt); guard_one(x.z, acc, cnt); guard_one(x.w, acc, cnt);
  }
  if (rel == 0) {
    if ((long)threadIdx.x < head) guard_one(a.p[threadIdx.x], acc, cnt);
    if ((long)threadIdx.x < tail) guard_one(a.p[head + 4 * nvec + threadIdx.x], acc, cnt);
  }
  const double bs = block_sum<kGuardWaves>(acc, s_d);
  const long long bc = block_sum<kGuardWaves>(cnt, s_c);
  if (threadIdx.x == 0) {
    GuardSlot o;
    o.sumsq = bs; o.nonfinite = bc;
    g.slots[blockIdx.x] = o;
  }
}

__global__ __launch_bounds__(kGuardThreads) void grad_guard_decide_kernel(const GuardSlot* slots, long n_slots, double max_norm, GuardState* st) {
  __shared__ double s_d[kGuardWaves];
  __shared__ long long s_c[kGuardWaves];
  double acc = 0.0;
  long long cnt = 0;
  for (long i = threadIdx.x; i < n_slots; i += kGuardThreads) { acc += slots[i].sumsq; cnt += slots[i].nonfinite; }
  const double sumsq = block_sum<kGuardWaves>(acc, s_d);
  const long long bad = block_sum<kGuardWaves>(cnt, s_c);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(sumsq);
  GuardState s = *st;
  s.steps += 1;
  s.last_norm = norm;                                   // (of the finite elements, when some are not)
  s.last_nonfinite = bad;
  if (bad > 0) {
    s.skip = 1; s.scale = 1.f;
    s.skipped += 1;
  } else {
    double coef = 1.0;
    if (max_norm > 0.0 && norm > 0.0) { coef = max_norm / (norm + 1e-6); coef = coef < 1.0 ? coef : 1.0; }     // torch.nn.utils.clip_grad_norm_
    s.skip = 0; s.scale = (float)coef;                  // rounded once
    if (s.scale < 1.f) s.clipped += 1;
    s.norm_sum += norm;
    s.norm_max = norm > s.norm_max ? norm : s.norm_max;
  }
  *st = s;
}

struct SgdGuardedArgs {
  float* w; float* mom; const float* grad; unsigned short* w_bf16;
  long n;
  float lr, momentum, wd, rescale, clip;
  const GuardState* st;
};

// The arithmetic of sgd_update_kernel spelled out operation by operation, in the order that kernel is compiled to (product, fused wd w +,
// product by lr, fused momentum mom -, sum), so that neither kernel's result depends on what the compiler contracts: with scale == 1.0f
// and no clipping the extra product is exact and the two kernels give the same bits.
__global__ __launch_bounds__(256) void sgd_update_guarded_kernel(SgdGuardedArgs g) {
  if (g.st->skip != 0) return;
  const float scale = g.st->scale, c = g.clip;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < g.n; i += (long)gridDim.x * 256) {
    const float w = g.w[i];
    float t = __fmul_rn(__fmul_rn(g.rescale, g.grad[i]), scale);
    if (c >= 0.f) t = fminf(fmaxf(t, -c), c);
    t = __fmul_rn(g.lr, __fmaf_rn(g.wd, w, t));
    const float m = __fmaf_rn(g.momentum, g.mom[i], -t);
    const float wn = __fadd_rn(w, m);
    g.mom[i] = m;
    g.w[i] = wn;
    if (g.w_bf16) g.w_bf16[i] = f2bf(wn);
  }
}

}  // namespace relnet

using namespace relnet;

extern "C" long relnet_grad_guard_workspace_bytes(long slots) { return slots < 1 ? 0 : slots * (long)sizeof(GuardSlot); }

extern "C" long relnet_grad_stats_slots(const long* ns, int n) {
  if (!ns || n < 1 || n > kGuardMaxRanges) return -1;
  long total = 0;
  for (int i = 0; i < n; ++i) {
    if (ns[i] < 1) return -1;
    total += guard_range_blocks(ns[i]);
  }
  return total;
}

extern "C" int relnet_grad_stats(const float* const* ptrs, const long* ns, int n, void* workspace, long slot_base, long slot_capacity,
                                 void* stream) {
  RELNET_REQUIRE(ptrs && ns && workspace, "relnet_grad_stats: null operand");
  RELNET_REQUIRE(n > 0 && n <= kGuardMaxRanges, "relnet_grad_stats: 1..%d ranges, got %d", kGuardMaxRanges, n);
  RELNET_REQUIRE(((uintptr_t)workspace & 15) == 0, "relnet_grad_stats: the workspace must be 16-byte aligned");
  StatsGroup g;
  g.n = n;
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    RELNET_REQUIRE(ptrs[i] && ns[i] > 0 && ((uintptr_t)ptrs[i] & 3) == 0, "relnet_grad_stats: range %d needs a 4-byte aligned pointer and n >= 1", i);
    StatsRange& r = g.r[i];
    r.p = ptrs[i]; r.n = ns[i];
    r.blk_start = (int)blocks;
    r.blocks = (int)guard_range_blocks(ns[i]);
    blocks += r.blocks;
  }
  RELNET_REQUIRE(slot_base >= 0 && slot_base + blocks <= slot_capacity, "relnet_grad_stats: slots %ld .. %ld do not fit a workspace of %ld",
                 slot_base, slot_base + blocks, slot_capacity);
  g.slots = (GuardSlot*)workspace + slot_base;
  grad_stats_kernel<<<(unsigned)blocks, kGuardThreads, 0, (hipStream_t)stream>>>(g);
  return check_launch("relnet_grad_stats");
}

extern "C" int relnet_grad_guard_decide(const void* workspace, long n_slots, double max_norm, void* state, void* stream) {
  RELNET_REQUIRE(workspace && state, "relnet_grad_guard_decide: null operand");
  RELNET_REQUIRE(n_slots > 0, "relnet_grad_guard_decide: no statistics slots (%ld)", n_slots);
  RELNET_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)state & 7) == 0,
                 "relnet_grad_guard_decide: the workspace must be 16-byte and the state 8-byte aligned");
  RELNET_REQUIRE(max_norm == max_norm, "relnet_grad_guard_decide: max_norm is NaN");
  grad_guard_decide_kernel<<<1, kGuardThreads, 0, (hipStream_t)stream>>>((const GuardSlot*)workspace, n_slots, max_norm, (GuardState*)state);
  return check_launch("relnet_grad_guard_decide");
}

extern "C" int relnet_sgd_update_guarded(float* w, float* mom, const float* grad, void* w_bf16, long n, float lr, float momentum, float wd,
                                         float rescale_grad, const void* state, float clip_gradient, void* stream) {
  RELNET_REQUIRE(w && mom && grad && state && n > 0, "relnet_sgd_update_guarded: bad operand");
  RELNET_REQUIRE(((uintptr_t)state & 7) == 0, "relnet_sgd_update_guarded: the state must be 8-byte aligned");
  RELNET_REQUIRE(clip_gradient == clip_gradient, "relnet_sgd_update_guarded: clip_gradient is NaN");
  SgdGuardedArgs g{w, mom, grad, (unsigned short*)w_bf16, n, lr, momentum, wd, rescale_grad, clip_gradient, (const GuardState*)state};
  long blocks = (n + 255) / 256;
  blocks = blocks > 8192 ? 8192 : blocks;
  sgd_update_guarded_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(g);
  return check_launch("relnet_sgd_update_guarded");
}
