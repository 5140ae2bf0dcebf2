// Proposal recall on the device (dataset/recall.py, the reference's lib/dataset/imdb.py:274-370 evaluate_recall): for one batch
// of candidate lists, the greedy cover of every image's valid ground truth per gt-area range, accumulated as integer counts.
//
// One workgroup per (batch image, area range).  The image's candidates are optionally divided by the image scale in fp32
// (numpy's float32_array / float(scale), correctly rounded) and kept when score > thresh (float32 compare, as numpy compares a
// float32 array with a Python float), in list order; they sit in LDS as float32.  The range's ground truth (the rows whose
// area-range bit is set: the host computes those bits once, in the roidb's dtype, which is where coco's uint16 areas wrap
// modulo 65536) sits in LDS as float64.
//
// The cover follows the reference exactly.  Per gt column the first (lowest proposal index) maximum over the unused proposals
// is cached.  A round takes the gt with the largest cached value, the LOWEST gt index on ties, and that gt's cached proposal:
// numpy's max_overlaps.argmax() then argmax_overlaps[gt_ind].  The proposal and the gt are marked used (the reference's -1 row
// and column); only the columns whose cached proposal was the one just used are rescanned.  min(P, G) rounds; with P < G the
// remaining entries are 0 and compared with the thresholds as 0.  IoU is bbox.pyx:15-55 in float64 with contraction off:
// iw = min(x2) - max(x1) + 1, ih only when iw > 0, ua = proposal area + gt area - iw * ih, iw * ih / ua, where min / max are
// Python's (the first operand unless the second is strictly smaller / larger).
//
// Outputs, all accumulated with integer atomics so that any batching gives the same numbers: hits[a, t] = recorded values
// >= thr[t], num_pos[a] = valid gts of range a (also of images without candidates), area_count[a - 1] = candidates with area
// (fp32, (x2 - x1 + 1) * (y2 - y1 + 1)) in [lo, hi) of range a >= 1.  Per image: n_cand = kept candidates, added += 1, and
// optionally the recorded values of each range in round order (overlaps [n_images, A, gt_cap] float64).
#include "common.h"

namespace relnet {

constexpr int kRecallThreads = 256;      // one lane per gt in the round's argmax
constexpr int kRecallWaves = kRecallThreads / kWave;
constexpr int kRecallMaxCand = 2048;     // candidates per image (LDS: 16 bytes each)
constexpr int kRecallMaxGt = 256;        // valid gt per image
constexpr int kRecallMaxThr = 256;       // IoU thresholds (one lane each)
constexpr int kRecallMaxAreas = 8;       // area ranges (one bit each)
constexpr int kCandPerThread = kRecallMaxCand / kRecallThreads;

struct RecallArgs {
  const float* boxes;               // [B, P, 4] with strides (box_bs, box_rs) in floats, x1 y1 x2 y2 contiguous
  long box_bs, box_rs;
  const float* scores;              // [B, P] or null
  const int* num_valid;             // [B] or null (all P)
  const float* scale;               // [B] or null
  float thresh;                     // used with scores
  const int* image_pos;             // [B]
  const int* gt_off;                // [n_images + 1]
  const double* gt_box;             // [n_gt, 4]
  const unsigned char* gt_mask;     // [n_gt] bit a: area in range a
  const double* thr;                // [T]
  const double* area_rng;           // [A, 2] half-open [lo, hi)
  unsigned long long* hits;         // [A, T]
  unsigned long long* num_pos;      // [A]
  unsigned long long* area_count;   // [A - 1]
  int* n_cand;                      // [n_images]
  int* added;                       // [n_images]
  double* overlaps;                 // [n_images, A, gt_cap] or null
  int B, P, n_images, A, T, gt_cap;
};

#pragma clang fp contract(off)
// Python's min / max on two numbers
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// bbox.pyx: overlap of proposal c with gt g (g_area = (x2 - x1 + 1) * (y2 - y1 + 1) of the gt)
__device__ __forceinline__ double recall_iou(const float4 c, const double* g, double g_area) {
  const double x1 = c.x, y1 = c.y, x2 = c.z, y2 = c.w;
  const double iw = py_min(x2, g[2]) - py_max(x1, g[0]) + 1.0;
  if (iw > 0.0) {
    const double ih = py_min(y2, g[3]) - py_max(y1, g[1]) + 1.0;
    if (ih > 0.0) {
      const double ua = (x2 - x1 + 1.0) * (y2 - y1 + 1.0) + g_area - iw * ih;
      return iw * ih / ua;
    }
  }
  return 0.0;
}

// (value desc, index asc): is (v, i) before (w, j)?
__device__ __forceinline__ bool recall_before(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

__device__ __forceinline__ void wave_best(double& v, int& i) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double w = __shfl_xor(v, off);
    const int j = __shfl_xor(i, off);
    if (recall_before(w, j, v, i)) { v = w; i = j; }
  }
}

// Exclusive prefix sum of one int per lane over the workgroup; *total gets the sum.  Contains two barriers.
__device__ __forceinline__ int block_exclusive_scan(int x, int* s_part, int* total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int inc = x;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  if (lane == kWave - 1) s_part[wave] = inc;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kRecallWaves; ++w) {
    before += w < wave ? s_part[w] : 0;
    sum += s_part[w];
  }
  *total = sum;
  __syncthreads();
  return before + inc - x;
}

// First maximum of gt column g over the unused candidates, by one wave: -> (value, proposal), value -2 when none is left.
__device__ __forceinline__ void column_best(const float4* s_box, const unsigned char* s_pused, int n, const double* g, double g_area,
                                            double& v, int& p) {
  const int lane = threadIdx.x & (kWave - 1);
  v = -2.0;
  p = 0x7fffffff;
  for (int i = lane; i < n; i += kWave) {
    if (s_pused[i]) continue;
    const double o = recall_iou(s_box[i], g, g_area);
    if (o > v) { v = o; p = i; }                          // i ascends in this lane: the first of equal values stays
  }
  wave_best(v, p);
}

__global__ __launch_bounds__(kRecallThreads) void recall_match_kernel(RecallArgs g) {
  __shared__ float4 s_box[kRecallMaxCand];
  __shared__ unsigned char s_pused[kRecallMaxCand];
  __shared__ double s_gt[kRecallMaxGt * 4];
  __shared__ double s_garea[kRecallMaxGt];
  __shared__ double s_bv[kRecallMaxGt];                   // cached column maximum (-1: gt used)
  __shared__ int s_bp[kRecallMaxGt];                      // its first proposal
  __shared__ double s_rec[kRecallMaxGt];                  // value recorded in round j
  __shared__ double s_wv[kRecallWaves];
  __shared__ int s_wi[kRecallWaves];
  __shared__ int s_part[kRecallWaves];
  __shared__ int s_count;

  const int b = blockIdx.x, a = blockIdx.y;
  const int img = g.image_pos[b];
  if (img < 0 || img >= g.n_images) return;
  const int g0 = g.gt_off[img], ng_img = g.gt_off[img + 1] - g0;
  if (ng_img < 0 || ng_img > kRecallMaxGt) return;        // the host refuses such a table before launch
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  // ---- candidates: scale, score filter, stable compaction into LDS
  int nv = g.num_valid ? g.num_valid[b] : g.P;
  nv = nv < 0 ? 0 : (nv > g.P ? g.P : nv);
  const float sc = g.scale ? g.scale[b] : 1.0f;
  float4 mine[kCandPerThread];
  unsigned keep = 0;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < kCandPerThread; ++k) {
    const int i = tid * kCandPerThread + k;
    if (i < nv) {
      const float* r = g.boxes + (long)b * g.box_bs + (long)i * g.box_rs;
      float4 c = make_float4(r[0], r[1], r[2], r[3]);
      if (g.scale) c = make_float4(__fdiv_rn(c.x, sc), __fdiv_rn(c.y, sc), __fdiv_rn(c.z, sc), __fdiv_rn(c.w, sc));
      const bool k_ok = g.scores == nullptr || g.scores[(long)b * g.P + i] > g.thresh;
      mine[k] = c;
      if (k_ok) { keep |= 1u << k; ++cnt; }
    } else {
      mine[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  int n = 0;
  int pos = block_exclusive_scan(cnt, s_part, &n);
#pragma unroll
  for (int k = 0; k < kCandPerThread; ++k) {
    if (keep & (1u << k)) {
      s_box[pos] = mine[k];
      s_pused[pos] = 0;
      ++pos;
    }
  }
  // ---- the range's ground truth, in roidb order
  const bool in_a = tid < ng_img && ((g.gt_mask[g0 + tid] >> a) & 1);
  int G = 0;
  const int gpos = block_exclusive_scan(in_a ? 1 : 0, s_part, &G);
  if (in_a) {
    const double* src = g.gt_box + 4 * (long)(g0 + tid);
    const double x1 = src[0], y1 = src[1], x2 = src[2], y2 = src[3];
    s_gt[4 * gpos + 0] = x1; s_gt[4 * gpos + 1] = y1; s_gt[4 * gpos + 2] = x2; s_gt[4 * gpos + 3] = y2;
    s_garea[gpos] = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
  }
  if (tid == 0) s_count = 0;
  __syncthreads();                                        // s_box, s_gt ready

  // ---- per-image counts
  if (a == 0) {
    if (tid == 0) {
      g.n_cand[img] = n;
      atomicAdd(&g.added[img], 1);
    }
  } else {
    const double lo = g.area_rng[2 * a], hi = g.area_rng[2 * a + 1];
    int c = 0;
    for (int i = tid; i < n; i += kRecallThreads) {
      const float4 q = s_box[i];
      const float area = (q.z - q.x + 1.0f) * (q.w - q.y + 1.0f);
      c += ((double)area >= lo && (double)area < hi) ? 1 : 0;
    }
    if (c) atomicAdd(&s_count, c);
  }
  if (tid == 0 && G) atomicAdd(&g.num_pos[a], (unsigned long long)G);
  if (n == 0 || G == 0) {                                 // the reference's `continue`, or nothing to cover
    __syncthreads();
    if (a > 0 && tid == 0 && s_count) atomicAdd(&g.area_count[a - 1], (unsigned long long)s_count);
    return;
  }

  // ---- initial column maxima
  for (int k = wave; k < G; k += kRecallWaves) {
    double v; int p;
    column_best(s_box, s_pused, n, s_gt + 4 * k, s_garea[k], v, p);
    if (lane == 0) { s_bv[k] = v; s_bp[k] = p; }
  }
  __syncthreads();
  const int rounds = n < G ? n : G;
  for (int j = 0; j < rounds; ++j) {
    // the gt with the largest column maximum, lowest index first
    double v = tid < G ? s_bv[tid] : -3.0;
    int gi = tid;
    wave_best(v, gi);
    if (lane == 0) { s_wv[wave] = v; s_wi[wave] = gi; }
    __syncthreads();
    v = s_wv[0]; gi = s_wi[0];
#pragma unroll
    for (int w = 1; w < kRecallWaves; ++w)
      if (recall_before(s_wv[w], s_wi[w], v, gi)) { v = s_wv[w]; gi = s_wi[w]; }
    const int pstar = s_bp[gi];
    __syncthreads();                                      // every lane has read s_bp[gi] and the wave results
    if (tid == 0) {
      s_rec[j] = v;
      s_pused[pstar] = 1;
      s_bv[gi] = -1.0;
    }
    __syncthreads();
    if (j + 1 < rounds) {
      for (int k = wave; k < G; k += kRecallWaves) {
        if (s_bv[k] == -1.0 || s_bp[k] != pstar) continue;      // used, or its maximum is still there
        double w; int p;
        column_best(s_box, s_pused, n, s_gt + 4 * k, s_garea[k], w, p);
        if (lane == 0) { s_bv[k] = w; s_bp[k] = p; }
      }
    }
    __syncthreads();
  }
  for (int k = rounds + tid; k < G; k += kRecallThreads) s_rec[k] = 0.0;
  __syncthreads();

  // ---- counts at every threshold, and the recorded values
  if (tid < g.T) {
    const double t = g.thr[tid];
    unsigned long long c = 0;
    for (int k = 0; k < G; ++k) c += s_rec[k] >= t ? 1 : 0;
    if (c) atomicAdd(&g.hits[(long)a * g.T + tid], c);
  }
  if (a > 0 && tid == 0 && s_count) atomicAdd(&g.area_count[a - 1], (unsigned long long)s_count);
  if (g.overlaps) {
    double* o = g.overlaps + ((long)img * g.A + a) * g.gt_cap;
    for (int k = tid; k < G && k < g.gt_cap; k += kRecallThreads) o[k] = s_rec[k];
  }
}
#pragma clang fp contract(on)

}  // namespace relnet

using namespace relnet;

extern "C" int relnet_recall_match(const float* boxes, long box_bs, long box_rs, const float* scores, const int* num_valid,
                                   const float* scale, float thresh, const int* image_pos, const int* gt_off, const double* gt_box,
                                   const unsigned char* gt_mask, const double* thresholds, const double* area_rng,
                                   unsigned long long* hits, unsigned long long* num_pos, unsigned long long* area_count,
                                   int* n_cand, int* added, double* overlaps, int B, int P, int n_images, int A, int T,
                                   int gt_cap, void* stream) {
  RELNET_REQUIRE(image_pos && gt_off && thresholds && area_rng && hits && num_pos && area_count && n_cand && added,
                 "relnet_recall_match: null operand");
  RELNET_REQUIRE(P == 0 || boxes, "relnet_recall_match: null boxes");
  RELNET_REQUIRE(gt_cap == 0 || (gt_box && gt_mask), "relnet_recall_match: null ground-truth operand");
  RELNET_REQUIRE(B > 0 && P >= 0 && n_images > 0 && A > 1 && T > 0 && gt_cap >= 0 && box_rs >= 4 && box_bs >= 0,
                 "relnet_recall_match: bad shape (B %d, P %d, n_images %d, A %d, T %d, gt_cap %d)", B, P, n_images, A, T,
                 gt_cap);
  RELNET_REQUIRE(P <= kRecallMaxCand, "relnet_recall_match: %d candidates per image, at most %d", P, kRecallMaxCand);
  RELNET_REQUIRE(gt_cap <= kRecallMaxGt, "relnet_recall_match: %d ground-truth boxes in one image, at most %d", gt_cap,
                 kRecallMaxGt);
  RELNET_REQUIRE(A <= kRecallMaxAreas && T <= kRecallMaxThr, "relnet_recall_match: %d area ranges (at most %d), %d thresholds "
                 "(at most %d)", A, kRecallMaxAreas, T, kRecallMaxThr);
  RecallArgs g;
  g.boxes = boxes; g.box_bs = box_bs; g.box_rs = box_rs; g.scores = scores; g.num_valid = num_valid; g.scale = scale;
  g.thresh = thresh; g.image_pos = image_pos; g.gt_off = gt_off; g.gt_box = gt_box; g.gt_mask = gt_mask; g.thr = thresholds;
  g.area_rng = area_rng; g.hits = hits; g.num_pos = num_pos; g.area_count = area_count; g.n_cand = n_cand; g.added = added;
  g.overlaps = overlaps; g.B = B; g.P = P; g.n_images = n_images; g.A = A; g.T = T; g.gt_cap = gt_cap;
  recall_match_kernel<<<dim3((unsigned)B, (unsigned)A), kRecallThreads, 0, (hipStream_t)stream>>>(g);
  return check_launch("relnet_recall_match");
}
