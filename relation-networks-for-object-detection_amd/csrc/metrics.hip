// Training metrics on the device (metric.py; the reference's relation_rcnn/core/metric.py): the numbers the reference logs every
// `frequent` batches, accumulated into a caller-owned buffer by launches that allocate nothing and never synchronise, so that they
// are captured into the step's hipGraph and keep counting on every replay.
//
// Every entry ADDS into slots the caller points at: integer slots (int64) with one 64-bit integer atomic per workgroup, float
// sums (double) without any floating-point atomic -- a float atomic sum depends on the order of arrival.  A sum is reduced per
// wave with shuffles (fixed tree), per workgroup through LDS (wave order), the workgroup's partial goes to a slab in the
// caller's workspace with a device-coherent store, and the workgroup that arrives last at the workspace's counter adds the
// partials in workgroup order and adds that total to the slot.  The grid is a function of the element count alone, each thread's
// elements are a function of the grid: the same inputs give the same bits on every run.  The last arriver also resets the
// counter, so a workspace is zeroed once, when it is created.  Launches that share a workspace must be ordered by their stream
// (the trainers keep one workspace per branch: RPN metrics on the side stream, the others on the main stream).
#include "common.h"
#include "wave.h"

namespace relnet {

constexpr int kMetricThreads = 256;
constexpr int kMetricWaves = kMetricThreads / kWave;
constexpr int kMetricMaxBlocks = 128;                    // partials per slab
constexpr int kMetricSlabs = 2;
constexpr long kMetricWorkspaceBytes = 64 + (long)kMetricSlabs * kMetricMaxBlocks * 8;   // counter (own 64 bytes) | slabs of doubles

struct MetricWorkspace {
  unsigned int* counter;
  unsigned long long* slab;                              // [kMetricSlabs][kMetricMaxBlocks] doubles as bit patterns
};

__device__ __forceinline__ MetricWorkspace metric_ws(void* p) {
  MetricWorkspace w;
  w.counter = (unsigned int*)p;
  w.slab = (unsigned long long*)((char*)p + 64);
  return w;
}

// Deterministic cross-workgroup fold of up to kMetricSlabs double partials per workgroup (thread 0 holds them).  Every
// workgroup stores its partials device-coherently, waits for them, and counts in; the last one to arrive reads all partials
// back (device-coherent loads), adds them in workgroup order and adds the totals to the slots.  Must be reached by every
// thread of every workgroup.
template <int NS>
__device__ __forceinline__ void fold_and_add(MetricWorkspace ws, const double (&part)[NS], double* const (&slot)[NS], double* s_fold,
                                             unsigned int* s_flag) {
  const int tid = threadIdx.x;
  const unsigned nb = gridDim.x;
  if (nb == 1) {                                          // (one workgroup: nothing to exchange)
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (slot[k]) *slot[k] += part[k];
    }
    return;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
      __hip_atomic_store(ws.slab + k * kMetricMaxBlocks + blockIdx.x, (unsigned long long)__double_as_longlong(part[k]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(ws.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old == nb - 1;
    if (last) __hip_atomic_store(ws.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
    *s_flag = last ? 1u : 0u;
  }
  __syncthreads();
  if (*s_flag == 0u) return;
  for (int i = tid; i < NS * kMetricMaxBlocks; i += kMetricThreads) {
    const int k = i / kMetricMaxBlocks, b = i - k * kMetricMaxBlocks;
    s_fold[i] = (unsigned)b < nb ? __longlong_as_double((long long)__hip_atomic_load(ws.slab + k * kMetricMaxBlocks + b, __ATOMIC_RELAXED,
                                                                                      __HIP_MEMORY_SCOPE_AGENT))
                                 : 0.0;
  }
  __syncthreads();
  if (tid < NS && slot[tid < NS ? tid : 0]) {             // one thread per slab, workgroup order
    double t = 0.0;
    for (unsigned b = 0; b < nb; ++b) t += s_fold[tid * kMetricMaxBlocks + b];
    *slot[tid] += t;
  }
}

// numpy's argmax order: is value v (class i) ahead of w (class j)?  The first of equal maxima wins; a NaN counts as the maximum.
__device__ __forceinline__ bool argmax_before(float v, int i, float w, int j) {
  const bool vn = v != v, wn = w != w;
  if (vn || wn) return vn && (!wn || i < j);
  return v > w || (v == w && i < j);
}

// -log(float32(p + 1e-14)) in double (metric.py:107-108: `cls += 1e-14` is a float32 add)
__device__ __forceinline__ double log_loss_term(float p) { return -log((double)__fadd_rn(p, 1e-14f)); }

struct SoftmaxMetricArgs {
  const float* prob;                // [outer, C, inner]
  const float* label;               // [outer * inner], float class ids, int32(label) == -1: ignored
  long outer, inner;
  int C;
  long long* correct;               // += #(argmax == label)
  long long* inst;                  // += #(label != -1)
  double* logloss;                  // += sum of -log(p[label] + 1e-14)
  void* ws;
};

// inner > 1 (the RPN's [B, 2, A h w]): one thread per position, the class stride is `inner`, so a wave reads 64 consecutive floats
// per class.  C == 2 with VEC 4 / VEC 2: four / two consecutive positions per thread with 16-byte / 8-byte loads (inner % VEC == 0, so a
// thread's positions lie in one image, and operands aligned to the load; 9 anchors on an odd-sized map are even, never a multiple of 4).
template <int VEC>
__global__ __launch_bounds__(kMetricThreads) void metric_softmax_inner_kernel(SoftmaxMetricArgs g) {
  __shared__ double s_d[kMetricWaves];
  __shared__ long long s_c[kMetricWaves], s_i[kMetricWaves];
  __shared__ double s_fold[kMetricMaxBlocks];
  __shared__ unsigned int s_flag;
  long long correct = 0, inst = 0;
  double loss = 0.0;
  const long total = g.outer * g.inner / VEC;
  for (long t = (long)blockIdx.x * kMetricThreads + threadIdx.x; t < total; t += (long)gridDim.x * kMetricThreads) {
    const long p = t * VEC;
    const long o = p / g.inner, i = p - o * g.inner;
    const float* base = g.prob + o * g.C * g.inner + i;
    if constexpr (VEC > 1) {
      typedef float vec_t __attribute__((ext_vector_type(VEC)));
      const vec_t lv = *(const vec_t*)(g.label + p);
      const vec_t av = *(const vec_t*)base, bv = *(const vec_t*)(base + g.inner);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const int lab = (int)lv[q];
        if (lab == -1) continue;
        ++inst;
        const int am = argmax_before(bv[q], 1, av[q], 0) ? 1 : 0;
        correct += am == lab ? 1 : 0;
        loss += log_loss_term(lab == 0 ? av[q] : lab == 1 ? bv[q] : 0.f);
      }
    } else {
      const int lab = (int)g.label[p];
      if (lab == -1) continue;
      ++inst;
      float best = base[0], pl = lab == 0 ? best : 0.f;
      int am = 0;
      for (int c = 1; c < g.C; ++c) {
        const float v = base[(long)c * g.inner];
        if (argmax_before(v, c, best, am)) { best = v; am = c; }
        if (c == lab) pl = v;
      }
      correct += am == lab ? 1 : 0;
      loss += log_loss_term(pl);                         // (a label outside [0, C) reads nothing: p = 0)
    }
  }
  const long long bc = block_sum<kMetricWaves>(correct, s_c), bi = block_sum<kMetricWaves>(inst, s_i);
  const double part[1] = {block_sum<kMetricWaves>(loss, s_d)};
  if (threadIdx.x == 0) {
    if (bc) atomicAdd((unsigned long long*)g.correct, (unsigned long long)bc);
    if (bi) atomicAdd((unsigned long long*)g.inst, (unsigned long long)bi);
  }
  double* const slot[1] = {g.logloss};
  fold_and_add<1>(metric_ws(g.ws), part, slot, s_fold, &s_flag);
}

// inner == 1 (the head's [B R, 81]): one wave per row, lanes over the classes (coalesced), first maximum by a wave reduction.
__global__ __launch_bounds__(kMetricThreads) void metric_softmax_row_kernel(SoftmaxMetricArgs g) {
  __shared__ double s_d[kMetricWaves];
  __shared__ long long s_c[kMetricWaves], s_i[kMetricWaves];
  __shared__ double s_fold[kMetricMaxBlocks];
  __shared__ unsigned int s_flag;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  long long correct = 0, inst = 0;                       // lane 0 of every wave counts
  double loss = 0.0;
  for (long r = (long)blockIdx.x * kMetricWaves + wave; r < g.outer; r += (long)gridDim.x * kMetricWaves) {
    const int lab = (int)g.label[r];
    if (lab == -1) continue;                             // (wave-uniform)
    const float* row = g.prob + r * g.C;
    float best = 0.f;
    int am = 0x7fffffff;                                 // no class yet: anything is ahead of it
    for (int c = lane; c < g.C; c += kWave) {
      const float v = row[c];
      if (am == 0x7fffffff || argmax_before(v, c, best, am)) { best = v; am = c; }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float w = __shfl_xor(best, off);
      const int j = __shfl_xor(am, off);
      if (j != 0x7fffffff && (am == 0x7fffffff || argmax_before(w, j, best, am))) { best = w; am = j; }
    }
    if (lane == 0) {
      ++inst;
      correct += am == lab ? 1 : 0;
      loss += log_loss_term(lab >= 0 && lab < g.C ? row[lab] : 0.f);
    }
  }
  const long long bc = block_sum<kMetricWaves>(correct, s_c), bi = block_sum<kMetricWaves>(inst, s_i);
  const double part[1] = {block_sum<kMetricWaves>(loss, s_d)};
  if (threadIdx.x == 0) {
    if (bc) atomicAdd((unsigned long long*)g.correct, (unsigned long long)bc);
    if (bi) atomicAdd((unsigned long long*)g.inst, (unsigned long long)bi);
  }
  double* const slot[1] = {g.logloss};
  fold_and_add<1>(metric_ws(g.ws), part, slot, s_fold, &s_flag);
}

struct SumCountArgs {
  const float* x;                   // [n]
  const float* x2;                  // [n] or null
  long n;
  const float* label;               // [n_label] or null; counted when label != -1 (a float compare, metric.py:154,178)
  long n_label;
  long long inst_inc;               // constant added to *count once per call
  double* sum;                      // += sum(x)
  double* sum2;                     // += sum(x2)
  long long* count;                 // += #(label != -1) + inst_inc
  void* ws;
};

// VEC 4: 16-byte loads over the aligned body (the entry point checks alignment), the last n % 4 elements by thread 0 of workgroup 0.
template <int VEC>
__global__ __launch_bounds__(kMetricThreads) void metric_sum_count_kernel(SumCountArgs g) {
  __shared__ double s_d[kMetricWaves], s_d2[kMetricWaves];
  __shared__ long long s_c[kMetricWaves];
  __shared__ double s_fold[kMetricSlabs * kMetricMaxBlocks];
  __shared__ unsigned int s_flag;
  const long first = (long)blockIdx.x * kMetricThreads + threadIdx.x, step = (long)gridDim.x * kMetricThreads;
  double a = 0.0, a2 = 0.0;
  long long cnt = 0;
  for (long t = first; t < g.n / VEC; t += step) {
    if constexpr (VEC == 4) {
      const float4 v = *((const float4*)g.x + t);
      a += (double)v.x; a += (double)v.y; a += (double)v.z; a += (double)v.w;
      if (g.x2) {
        const float4 w = *((const float4*)g.x2 + t);
        a2 += (double)w.x; a2 += (double)w.y; a2 += (double)w.z; a2 += (double)w.w;
      }
    } else {
      a += (double)g.x[t];
      if (g.x2) a2 += (double)g.x2[t];
    }
  }
  for (long t = first; t < g.n_label / VEC; t += step) {
    if constexpr (VEC == 4) {
      const float4 l = *((const float4*)g.label + t);
      cnt += (l.x != -1.f) + (l.y != -1.f) + (l.z != -1.f) + (l.w != -1.f);
    } else {
      cnt += g.label[t] != -1.f;
    }
  }
  if (VEC == 4 && first == 0) {
    for (long t = g.n / 4 * 4; t < g.n; ++t) {
      a += (double)g.x[t];
      if (g.x2) a2 += (double)g.x2[t];
    }
    for (long t = g.n_label / 4 * 4; t < g.n_label; ++t) cnt += g.label[t] != -1.f;
  }
  if (first == 0) cnt += g.inst_inc;
  const long long bc = block_sum<kMetricWaves>(cnt, s_c);
  const double part[2] = {block_sum<kMetricWaves>(a, s_d), block_sum<kMetricWaves>(a2, s_d2)};
  if (threadIdx.x == 0 && bc && g.count) atomicAdd((unsigned long long*)g.count, (unsigned long long)bc);
  double* const slot[2] = {g.sum, g.x2 ? g.sum2 : nullptr};
  fold_and_add<2>(metric_ws(g.ws), part, slot, s_fold, &s_flag);
}

// metric.py:231-248: strict compares against 0.5, an element equal to 0.5 is on neither side.  counts = {pos true, pos inst,
// neg true, neg inst}.
template <int VEC>
__global__ __launch_bounds__(kMetricThreads) void metric_nms_acc_kernel(const float* target, const float* cond, long n, long long* counts) {
  __shared__ long long s_c[4][kMetricWaves];
  long long c[4] = {0, 0, 0, 0};
  auto one = [&](float t, float s) {
    const bool tp = t > 0.5f, tn = t < 0.5f;
    c[1] += tp; c[0] += tp && s > 0.5f;
    c[3] += tn; c[2] += tn && s < 0.5f;
  };
  const long first = (long)blockIdx.x * kMetricThreads + threadIdx.x, step = (long)gridDim.x * kMetricThreads;
  for (long t = first; t < n / VEC; t += step) {
    if constexpr (VEC == 4) {
      const float4 a = *((const float4*)target + t), b = *((const float4*)cond + t);
      one(a.x, b.x); one(a.y, b.y); one(a.z, b.z); one(a.w, b.w);
    } else {
      one(target[t], cond[t]);
    }
  }
  if (VEC == 4 && first == 0)
    for (long t = n / 4 * 4; t < n; ++t) one(target[t], cond[t]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long v = wave_sum(c[k]);
    if ((threadIdx.x & (kWave - 1)) == 0) s_c[k][threadIdx.x / kWave] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < kMetricWaves; ++w) t += s_c[threadIdx.x][w];
    if (t) atomicAdd((unsigned long long*)counts + threadIdx.x, (unsigned long long)t);
  }
}

static unsigned metric_blocks(long work_items) {
  long b = (work_items + 4 * kMetricThreads - 1) / (4 * kMetricThreads);       // four items per thread before the grid grows
  return (unsigned)(b < 1 ? 1 : (b > kMetricMaxBlocks ? kMetricMaxBlocks : b));
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace relnet

using namespace relnet;

extern "C" long relnet_metric_workspace_bytes(void) { return kMetricWorkspaceBytes; }

extern "C" int relnet_metric_softmax(const float* prob, const float* label, long outer, int C, long inner, long long* correct,
                                     long long* inst, double* logloss, void* workspace, void* stream) {
  RELNET_REQUIRE(prob && label && correct && inst && logloss && workspace, "relnet_metric_softmax: null operand");
  RELNET_REQUIRE(outer > 0 && C > 0 && inner > 0, "relnet_metric_softmax: bad shape (outer %ld, C %d, inner %ld)", outer, C, inner);
  RELNET_REQUIRE((((uintptr_t)correct | (uintptr_t)inst | (uintptr_t)logloss | (uintptr_t)workspace) & 7) == 0,
                 "relnet_metric_softmax: accumulator slots and workspace must be 8-byte aligned");
  SoftmaxMetricArgs g;
  g.prob = prob; g.label = label; g.outer = outer; g.inner = inner; g.C = C; g.correct = correct; g.inst = inst; g.logloss = logloss;
  g.ws = workspace;
  hipStream_t s = (hipStream_t)stream;
  if (inner == 1) {
    metric_softmax_row_kernel<<<metric_blocks(outer * kWave), kMetricThreads, 0, s>>>(g);
  } else if (C == 2 && inner % 4 == 0 && aligned16(prob) && aligned16(label)) {
    metric_softmax_inner_kernel<4><<<metric_blocks(outer * inner / 4), kMetricThreads, 0, s>>>(g);
  } else if (C == 2 && inner % 2 == 0 && aligned8(prob) && aligned8(label)) {
    metric_softmax_inner_kernel<2><<<metric_blocks(outer * inner / 2), kMetricThreads, 0, s>>>(g);
  } else {
    metric_softmax_inner_kernel<1><<<metric_blocks(outer * inner), kMetricThreads, 0, s>>>(g);
  }
  return check_launch("relnet_metric_softmax");
}

extern "C" int relnet_metric_sum_count(const float* x, const float* x2, long n, const float* label, long n_label, long inst_inc,
                                       double* sum, double* sum2, long long* count, void* workspace, void* stream) {
  RELNET_REQUIRE(x && sum && workspace && n > 0, "relnet_metric_sum_count: null operand or empty tensor");
  RELNET_REQUIRE(!x2 || sum2, "relnet_metric_sum_count: a second tensor needs a second sum slot");
  RELNET_REQUIRE((label == nullptr) == (n_label == 0) && n_label >= 0 && inst_inc >= 0, "relnet_metric_sum_count: bad label operand");
  RELNET_REQUIRE(count || (!label && inst_inc == 0), "relnet_metric_sum_count: counting needs a count slot");
  RELNET_REQUIRE((((uintptr_t)sum | (uintptr_t)sum2 | (uintptr_t)count | (uintptr_t)workspace) & 7) == 0,
                 "relnet_metric_sum_count: accumulator slots and workspace must be 8-byte aligned");
  SumCountArgs g;
  g.x = x; g.x2 = x2; g.n = n; g.label = label; g.n_label = n_label; g.inst_inc = inst_inc; g.sum = sum; g.sum2 = sum2; g.count = count;
  g.ws = workspace;
  hipStream_t s = (hipStream_t)stream;
  const long items = n > n_label ? n : n_label;
  if (aligned16(x) && aligned16(x2) && aligned16(label))
    metric_sum_count_kernel<4><<<metric_blocks(items / 4 + 1), kMetricThreads, 0, s>>>(g);
  else
    metric_sum_count_kernel<1><<<metric_blocks(items), kMetricThreads, 0, s>>>(g);
  return check_launch("relnet_metric_sum_count");
}

extern "C" int relnet_metric_nms_acc(const float* target, const float* cond, long n, long long* counts, void* stream) {
  RELNET_REQUIRE(target && cond && counts && n > 0, "relnet_metric_nms_acc: null operand or empty tensor");
  RELNET_REQUIRE(((uintptr_t)counts & 7) == 0, "relnet_metric_nms_acc: the count slots must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (aligned16(target) && aligned16(cond))
    metric_nms_acc_kernel<4><<<metric_blocks(n / 4 + 1), kMetricThreads, 0, s>>>(target, cond, n, counts);
  else
    metric_nms_acc_kernel<1><<<metric_blocks(n), kMetricThreads, 0, s>>>(target, cond, n, counts);
  return check_launch("relnet_metric_nms_acc");
}
