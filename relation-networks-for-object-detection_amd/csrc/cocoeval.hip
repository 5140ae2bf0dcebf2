// COCO bbox evaluation on the device (dataset/cocoeval.py, the published pycocotools algorithm): per-image greedy matching of
// detections to ground truth for every (area range, IoU threshold) pair, then one stable sort of all matched detections by
// (category, -score) and the precision / recall accumulation per (category, area range, maxDets).
// Every float64 expression is evaluated in numpy's order with contraction off, so the precision and recall arrays are
// bit-identical to dataset/cocoeval.py.
#include "common.h"
#include "ordering.h"

namespace relnet {

constexpr int kCocoMatchThreads = 1024;      // the (category, area, threshold) loops of one image are latency-bound: many lanes
constexpr int kCocoMaxSlots = 2048;        // detection slots per image (LDS: 16 bytes per slot)
constexpr int kCocoMaxPairs = 64;          // area ranges x IoU thresholds (one lane each in the accumulation)
constexpr int kCocoMaxDetsLen = 4;         // entries of Params.maxDets
constexpr int kCocoMaxAreas = 7;           // area ranges (gt_flags: bit 0 iscrowd, bit 1 + a ignored in range a)
constexpr int kSortTile = 2048;            // elements per workgroup of one radix pass
constexpr int kSortThreads = 256;          // = radix

enum { kCodeFP = 0, kCodeTP = 1, kCodeIgnored = 2 };

struct CocoMatchArgs {
  const void* det;               // [B, S_in, 6] float32 or float64: class, score, then the box
  const int* num_det;            // [B]
  const int* image_pos;          // [B] position of the batch image in the evaluated image list
  const int* class_to_cat;       // [n_classes] category position or -1
  const int* gt_off;             // [n_images * K + 1] CSR over (image, category), annotation order inside a cell
  const double* gt_box;          // [n_gt, 4] x, y, w, h
  const unsigned char* gt_flags; // [n_gt] bit 0 iscrowd, bit 1 + a: ignored in area range a
  const double* iou_thr;         // [T]
  const double* area_rng;        // [A, 2] inclusive bounds
  unsigned char* gtm;            // [B, gt_cap, A * T] scratch: gt matched at (area, threshold)
  int* slot_cat;                 // [n_images, S]
  double* slot_score;            // [n_images, S]
  int* slot_rank;                // [n_images, S]
  unsigned char* slot_code;      // [n_images, S, A * T]
  int B, S_in, S, n_images, n_classes, K, A, T, gt_cap, max_det, f64, round_f32, xywh;
};

#pragma clang fp contract(off)
// One value of a detection row as results_list + COCOeval see it (pred_eval rounds float64 rows to float32 first).
__device__ __forceinline__ double det_value(const CocoMatchArgs& g, long idx) {
  if (g.f64) {
    const double v = ((const double*)g.det)[idx];
    return g.round_f32 ? (double)(float)v : v;
  }
  return (double)((const float*)g.det)[idx];
}

__device__ __forceinline__ void det_box(const CocoMatchArgs& g, long row, double& x, double& y, double& w, double& h) {
  x = det_value(g, row * 6 + 2);
  y = det_value(g, row * 6 + 3);
  const double c = det_value(g, row * 6 + 4), d = det_value(g, row * 6 + 5);
  if (g.xywh) {
    w = c; h = d;
  } else {                                  // coco.py:results_list, w = x2 - x1 + 1
    w = c - x + 1.0;
    h = d - y + 1.0;
  }
}

// dataset/cocoeval.py:bbox_iou for one pair, the same operations in the same order
__device__ __forceinline__ double coco_iou(double dx, double dy, double dw, double dh, const double* gb, bool crowd) {
  const double gx = gb[0], gy = gb[1], gw = gb[2], gh = gb[3];
  const double da = dw * dh, ga = gw * gh;
  const double dx2 = dx + dw, gx2 = gx + gw, dy2 = dy + dh, gy2 = gy + gh;
  const double w = (dx2 < gx2 ? dx2 : gx2) - (dx > gx ? dx : gx);
  const double h = (dy2 < gy2 ? dy2 : gy2) - (dy > gy ? dy : gy);
  const double inter = (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
  const double uni = crowd ? da : da + ga - inter;
  return inter / (uni > 1e-300 ? uni : 1e-300);
}

// Sort key of a score for numpy's argsort(-scores, kind='mergesort'): descending, -0.0 tied with 0.0, NaN after every number.
__device__ __forceinline__ unsigned long long desc_score_key(double s) {
  const unsigned long long u = order_key(s == 0.0 ? 0.0 : s);     // ascending order of s
  return s != s ? ~0ull : ~u;                                // descending (-inf: 0xfff0...0, below NaN); NaN: numpy sorts it last
}

// One workgroup per batch image.  LDS: category position and score of every row, then the rows in (category, -score, row)
// order.  One thread per (category of the image, area range, IoU threshold) runs that pair's greedy loop (_evaluate_img).
__global__ __launch_bounds__(kCocoMatchThreads) void coco_match_kernel(CocoMatchArgs g) {
  extern __shared__ double lds_d[];
  double* s_score = lds_d;                                   // [S_in]
  int* s_cat = (int*)(s_score + g.S_in);                     // [S_in]
  short* s_order = (short*)(s_cat + g.S_in);                 // [S_in] row at (image-local) sorted position
  short* s_group = s_order + g.S_in;                         // sorted position of each category's first row
  __shared__ int s_nvalid, s_ngroups;
  __shared__ double s_thr[kCocoMaxPairs], s_area[2 * kCocoMaxPairs];

  const int b = blockIdx.x;
  const int img = g.image_pos[b];
  if (img < 0 || img >= g.n_images) return;
  int n = g.num_det[b];
  n = n < 0 ? 0 : (n > g.S_in ? g.S_in : n);
  const int tid = threadIdx.x;
  if (tid == 0) { s_nvalid = 0; s_ngroups = 0; }
  if (tid < g.T) s_thr[tid] = g.iou_thr[tid] < 1.0 - 1e-10 ? g.iou_thr[tid] : 1.0 - 1e-10;
  if (tid < 2 * g.A) s_area[tid] = g.area_rng[tid];
  for (int i = tid; i < g.S_in; i += kCocoMatchThreads) {
    int cat = -1;
    double score = 0.0;
    if (i < n) {
      const long row = (long)b * g.S_in + i;
      const double cv = det_value(g, row * 6);
      if (cv >= 0.0 && cv < (double)g.n_classes) {
        const int cls = (int)cv;
        if ((double)cls == cv) cat = g.class_to_cat[cls];
      }
      score = det_value(g, row * 6 + 1);
    }
    s_cat[i] = cat;
    s_score[i] = score;
  }
  __syncthreads();
  // rank inside the (image, category) list after the stable descending sort, and the number of rows of lower categories
  int nv_local = 0;
  for (int i = tid; i < g.S_in; i += kCocoMatchThreads) {
    const int c = s_cat[i];
    if (c < 0) continue;
    const double sc = s_score[i];
    const unsigned long long kc = desc_score_key(sc);
    int rank = 0, before = 0;
    for (int j = 0; j < g.S_in; ++j) {
      const int cj = s_cat[j];
      if (cj < 0) continue;
      if (cj < c) {
        ++before;
      } else if (cj == c) {
        const unsigned long long kj = desc_score_key(s_score[j]);
        rank += (kj < kc || (kj == kc && j < i)) ? 1 : 0;
      }
    }
    const int pos = before + rank;
    s_order[pos] = (short)i;
    if (rank == 0) s_group[atomicAdd(&s_ngroups, 1)] = (short)pos;
    const long slot = (long)img * g.S + pos;
    g.slot_cat[slot] = c;
    g.slot_score[slot] = sc;
    g.slot_rank[slot] = rank;
    ++nv_local;
  }
  atomicAdd(&s_nvalid, nv_local);
  __syncthreads();
  const int nv = s_nvalid;
  for (int p = nv + tid; p < g.S; p += kCocoMatchThreads) {   // the image's remaining slots are empty
    const long slot = (long)img * g.S + p;
    g.slot_cat[slot] = -1;
    g.slot_score[slot] = 0.0;
    g.slot_rank[slot] = 0x7fffffff;
  }
  const int AT = g.A * g.T;
  const int units = s_ngroups * AT;
  const int gt_img0 = g.gt_off[(long)img * g.K];
  for (int u = tid; u < units; u += kCocoMatchThreads) {
    const int gpos = s_group[u / AT];
    const int pair = u % AT;
    const int a = pair / g.T, t = pair % g.T;
    const int c = s_cat[s_order[gpos]];
    const int g0 = g.gt_off[(long)img * g.K + c], g1 = g.gt_off[(long)img * g.K + c + 1];
    unsigned char* gtm = g.gtm + ((long)b * g.gt_cap + (g0 - gt_img0)) * AT + pair;
    for (int k = 0; k < g1 - g0; ++k) gtm[(long)k * AT] = 0;
    const double thr0 = s_thr[t];
    const double alo = s_area[2 * a], ahi = s_area[2 * a + 1];
    const unsigned char ig_bit = (unsigned char)(2u << a);
    for (int p = gpos; p < nv && p - gpos < g.max_det; ++p) {
      const int i = s_order[p];
      if (s_cat[i] != c) break;
      double dx, dy, dw, dh;
      det_box(g, (long)b * g.S_in + i, dx, dy, dw, dh);
      double best = thr0;
      int m = -1;
      bool m_ig = false;
      // ground truth in _evaluate_img's order: the regular boxes, then (only while nothing regular matched) the ignored ones
      for (int pass = 0; pass < 2 && m < 0; ++pass) {
        for (int k = 0; k < g1 - g0; ++k) {
          const unsigned char f = g.gt_flags[g0 + k];
          const bool ig = (f & ig_bit) != 0, crowd = (f & 1) != 0;
          if (ig != (pass == 1)) continue;
          if (gtm[(long)k * AT] && !crowd) continue;
          const double iou = coco_iou(dx, dy, dw, dh, g.gt_box + 4 * (long)(g0 + k), crowd);
          if (iou < best) continue;
          best = iou;
          m = k;
          m_ig = ig;
        }
      }
      unsigned char code;
      if (m >= 0) {
        gtm[(long)m * AT] = 1;
        code = m_ig ? kCodeIgnored : kCodeTP;
      } else {
        const double area = dw * dh;
        code = (area < alo || area > ahi) ? kCodeIgnored : kCodeFP;
      }
      g.slot_code[((long)img * g.S + p) * AT + pair] = code;
    }
  }
}

// ---- accumulate: one stable LSD radix sort of every slot by (category, -score), then one scan per category ----------------

__global__ __launch_bounds__(256) void coco_sort_init_kernel(const int* slot_cat, const double* slot_score, const int* slot_rank,
                                                             unsigned long long* key, int* val, int* catd, long n, int K,
                                                             int max_det) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = slot_cat[i];
  catd[i] = (c >= 0 && c < K && slot_rank[i] < max_det) ? c : K;
  key[i] = desc_score_key(slot_score[i]);
  val[i] = (int)i;
}

__global__ __launch_bounds__(256) void coco_rekey_kernel(const int* val, const int* catd, unsigned long long* key, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = (unsigned long long)catd[val[i]];
}

// per-tile digit counts, digit-major: hist[d * n_tiles + tile]
__global__ __launch_bounds__(kSortThreads) void coco_radix_hist_kernel(const unsigned long long* key, long n, int shift,
                                                                       int* hist, int n_tiles) {
  __shared__ int cnt[kSortThreads];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * kSortTile;
  for (int j = threadIdx.x; j < kSortTile; j += kSortThreads) {
    if (base + j < n) atomicAdd(&cnt[(key[base + j] >> shift) & 255], 1);
  }
  __syncthreads();
  hist[(long)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of hist[0, len) in place, one workgroup
__global__ __launch_bounds__(1024) void coco_scan_kernel(int* hist, long len) {
  __shared__ int part[1024];
  const long per = (len + 1023) / 1024;
  const long lo = threadIdx.x * per, hi = lo + per < len ? lo + per : len;
  int s = 0;
  for (long i = lo; i < hi; ++i) s += hist[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (long i = lo; i < hi; ++i) {
    const int v = hist[i];
    hist[i] = run;
    run += v;
  }
}

// Stable scatter: thread d walks the tile in order and places the elements of digit d at its running offset.
__global__ __launch_bounds__(kSortThreads) void coco_radix_scatter_kernel(const unsigned long long* key_in, const int* val_in,
                                                                          unsigned long long* key_out, int* val_out, long n,
                                                                          int shift, const int* hist, int n_tiles) {
  __shared__ unsigned int dig[kSortTile / 4];
  const long base = (long)blockIdx.x * kSortTile;
  const int cnt = (int)(n - base < kSortTile ? n - base : kSortTile);
  unsigned char* d8 = (unsigned char*)dig;
  for (int j = threadIdx.x; j < kSortTile; j += kSortThreads)
    d8[j] = j < cnt ? (unsigned char)((key_in[base + j] >> shift) & 255) : 0;
  __syncthreads();
  const unsigned d = threadIdx.x;
  int pos = hist[(long)d * n_tiles + blockIdx.x];
  for (int w = 0; w < (cnt + 3) / 4; ++w) {
    const unsigned int v = dig[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * w + q;
      if (j < cnt && ((v >> (8 * q)) & 255u) == d) {
        key_out[pos] = key_in[base + j];
        val_out[pos] = val_in[base + j];
        ++pos;
      }
    }
  }
}

// After the category passes key[i] is the category digit (K = not evaluated); seg[2k], seg[2k+1] = [start, end) of category k.
__global__ __launch_bounds__(256) void coco_segments_kernel(const unsigned long long* key, long n, int K, long* seg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long c = key[i];
  if (c >= (unsigned long long)K) return;
  if (i == 0 || key[i - 1] != c) seg[2 * c] = i;
  if (i == n - 1 || key[i + 1] != c) seg[2 * c + 1] = i + 1;
}

__global__ __launch_bounds__(256) void coco_gather_kernel(const unsigned long long* key, const int* val, const int* slot_rank,
                                                          const unsigned char* slot_code, int* srank, unsigned char* scode,
                                                          long n, int K, int AT) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || key[i] >= (unsigned long long)K) return;
  const long s = val[i];
  srank[i] = slot_rank[s];
  for (int p = 0; p < AT; ++p) scode[i * AT + p] = slot_code[s * AT + p];
}

struct CocoAccArgs {
  const long* seg;              // [K, 2]
  const int* srank;             // sorted
  const unsigned char* scode;   // sorted, [n, A*T]
  const long long* npig;        // [K, A]
  const double* rec_thr;        // [R]
  const int* max_dets;          // [M]
  double* precision;            // [T, R, K, A, M]
  double* recall;               // [T, K, A, M]
  int K, A, T, R, M;
};

// One workgroup per category; lane (a, t) accumulates all M maxDets cut-offs of that pair.  A forward pass counts the
// true / false positives; a backward pass rebuilds tp[i], fp[i], keeps the suffix maximum of the precision and assigns
// each recall threshold the suffix maximum at its left searchsorted index.
__global__ __launch_bounds__(64) void coco_accumulate_kernel(CocoAccArgs g) {
  const int k = blockIdx.x;
  const int pair = threadIdx.x;
  const int AT = g.A * g.T;
  if (pair >= AT) return;
  const int a = pair / g.T, t = pair % g.T;
  const long long npig = g.npig[(long)k * g.A + a];
  const long lo = g.seg[2 * k], hi = g.seg[2 * k + 1];
  const int M = g.M, R = g.R;
  auto P = [&](int r, int m) -> double& { return g.precision[((((long)t * R + r) * g.K + k) * g.A + a) * M + m]; };
  double* recall = g.recall + (((long)t * g.K + k) * g.A + a) * M;
  if (npig == 0) {
    for (int m = 0; m < M; ++m) {
      recall[m] = -1.0;
      for (int r = 0; r < R; ++r) P(r, m) = -1.0;
    }
    return;
  }
  int md[kCocoMaxDetsLen], tp[kCocoMaxDetsLen], fp[kCocoMaxDetsLen], nd[kCocoMaxDetsLen], hi_prev[kCocoMaxDetsLen];
  double smax[kCocoMaxDetsLen];
#pragma unroll
  for (int m = 0; m < kCocoMaxDetsLen; ++m) {
    md[m] = m < M ? g.max_dets[m] : 0;
    tp[m] = 0; fp[m] = 0; nd[m] = 0;
  }
  for (long i = lo; i < hi; ++i) {
    const int rk = g.srank[i];
    const unsigned char code = g.scode[i * AT + pair];
#pragma unroll
    for (int m = 0; m < kCocoMaxDetsLen; ++m) {
      if (rk < md[m]) {
        ++nd[m];
        tp[m] += code == kCodeTP;
        fp[m] += code == kCodeFP;
      }
    }
  }
  const double np = (double)npig;
#pragma unroll
  for (int m = 0; m < kCocoMaxDetsLen; ++m) {
    if (m >= M) continue;
    recall[m] = nd[m] ? (double)tp[m] / np : 0.0;
    hi_prev[m] = R;
    smax[m] = 0.0;                                          // precision beyond the last detection
  }
  for (long i = hi - 1; i >= lo; --i) {
    const int rk = g.srank[i];
    const unsigned char code = g.scode[i * AT + pair];
#pragma unroll
    for (int m = 0; m < kCocoMaxDetsLen; ++m) {
      if (m >= M || rk >= md[m]) continue;
      const double tpd = (double)tp[m], fpd = (double)fp[m];
      const double rc = tpd / np;
      const double pr = tpd / (fpd + tpd + 2.220446049250313e-16);
      int h = hi_prev[m];
      while (h > 0 && g.rec_thr[h - 1] > rc) --h;           // thresholds h..hi_prev-1 first reach rc at the next position
      for (int r = h; r < hi_prev[m]; ++r) P(r, m) = smax[m];
      hi_prev[m] = h;
      smax[m] = pr > smax[m] ? pr : smax[m];                 // pr >= +0.0: the first one replaces the 0 above
      tp[m] -= code == kCodeTP;
      fp[m] -= code == kCodeFP;
    }
  }
#pragma unroll
  for (int m = 0; m < kCocoMaxDetsLen; ++m) {
    if (m >= M) continue;
    for (int r = 0; r < hi_prev[m]; ++r) P(r, m) = smax[m];
  }
}
#pragma clang fp contract(on)

}  // namespace relnet

using namespace relnet;

extern "C" long relnet_coco_accumulate_workspace_bytes(long n_slots, int K, int pairs) {
  if (n_slots <= 0 || K <= 0 || pairs <= 0) return -1;
  const long tiles = (n_slots + kSortTile - 1) / kSortTile;
  long b = 0;
  b += 2 * 8 * n_slots;                       // keys, ping-pong
  b += 2 * 4 * n_slots;                       // values, ping-pong
  b += 4 * n_slots;                           // category digit
  b += 4 * 256 * tiles;                       // per-tile histograms
  b += 16 * (long)K;                          // segments
  b += 4 * n_slots + (long)pairs * n_slots;   // sorted ranks and codes
  return b + 16 * 256;                        // per-buffer alignment
}

extern "C" int relnet_coco_match(const void* det, int det_dtype, const int* num_det, const int* image_pos, const int* class_to_cat,
                                 const int* gt_off, const double* gt_box, const unsigned char* gt_flags, const double* iou_thr,
                                 const double* area_rng, void* gtm_scratch, int* slot_cat, double* slot_score, int* slot_rank,
                                 void* slot_code, int B, int S_in, int S, int n_images, int n_classes, int K, int A, int T,
                                 int gt_cap, int max_det, int round_f32, int box_xywh, void* stream) {
  RELNET_REQUIRE(det && num_det && image_pos && class_to_cat && gt_off && iou_thr && area_rng && slot_cat && slot_score &&
                 slot_rank && slot_code, "relnet_coco_match: null operand");
  RELNET_REQUIRE(gt_cap == 0 || (gt_box && gt_flags && gtm_scratch), "relnet_coco_match: null ground-truth operand");
  RELNET_REQUIRE(det_dtype == 0 || det_dtype == 1, "relnet_coco_match: detections must be float32 (0) or float64 (1)");
  RELNET_REQUIRE(B > 0 && S_in > 0 && S_in <= S && n_images > 0 && n_classes > 0 && K > 0 && A > 0 && T > 0 && gt_cap >= 0 &&
                 max_det > 0, "relnet_coco_match: bad shape (B %d, S_in %d, S %d, n_images %d, K %d, A %d, T %d)", B, S_in, S,
                 n_images, K, A, T);
  RELNET_REQUIRE(S <= kCocoMaxSlots, "relnet_coco_match: %d detection slots per image, at most %d", S, kCocoMaxSlots);
  RELNET_REQUIRE(A <= kCocoMaxAreas && A * T <= kCocoMaxPairs, "relnet_coco_match: %d area ranges (at most %d), %d (area, IoU) "
                 "pairs (at most %d)", A, kCocoMaxAreas, A * T, kCocoMaxPairs);
  CocoMatchArgs g;
  g.det = det; g.num_det = num_det; g.image_pos = image_pos; g.class_to_cat = class_to_cat; g.gt_off = gt_off;
  g.gt_box = gt_box; g.gt_flags = gt_flags; g.iou_thr = iou_thr; g.area_rng = area_rng; g.gtm = (unsigned char*)gtm_scratch;
  g.slot_cat = slot_cat; g.slot_score = slot_score; g.slot_rank = slot_rank; g.slot_code = (unsigned char*)slot_code;
  g.B = B; g.S_in = S_in; g.S = S; g.n_images = n_images; g.n_classes = n_classes; g.K = K; g.A = A; g.T = T;
  g.gt_cap = gt_cap; g.max_det = max_det; g.f64 = det_dtype == 1; g.round_f32 = round_f32 != 0; g.xywh = box_xywh != 0;
  const size_t lds = (size_t)S_in * (8 + 4 + 2 + 2);
  coco_match_kernel<<<(unsigned)B, kCocoMatchThreads, lds, (hipStream_t)stream>>>(g);
  return check_launch("relnet_coco_match");
}

extern "C" int relnet_coco_accumulate(const int* slot_cat, const double* slot_score, const int* slot_rank, const void* slot_code,
                                      long n_slots, const long long* npig, const double* rec_thr, const int* max_dets,
                                      double* precision, double* recall, void* workspace, long workspace_bytes, int K, int A,
                                      int T, int R, int M, int max_det_host, void* stream) {
  RELNET_REQUIRE(slot_cat && slot_score && slot_rank && slot_code && npig && rec_thr && max_dets && precision && recall &&
                 workspace, "relnet_coco_accumulate: null operand");
  RELNET_REQUIRE(n_slots > 0 && n_slots < (1l << 31) && K > 0 && K < 65535 && A > 0 && T > 0 && R > 0 && M > 0 &&
                 max_det_host > 0, "relnet_coco_accumulate: bad shape");
  RELNET_REQUIRE(A * T <= kCocoMaxPairs && M <= kCocoMaxDetsLen, "relnet_coco_accumulate: %d (area, IoU) pairs (at most %d), "
                 "%d maxDets (at most %d)", A * T, kCocoMaxPairs, M, kCocoMaxDetsLen);
  const int AT = A * T;
  const long need = relnet_coco_accumulate_workspace_bytes(n_slots, K, AT);
  RELNET_REQUIRE(workspace_bytes >= need, "relnet_coco_accumulate: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const long n = n_slots, tiles = (n + kSortTile - 1) / kSortTile;
  char* w = (char*)workspace;
  auto take = [&](long bytes) { char* p = w; w += (bytes + 255) / 256 * 256; return p; };
  unsigned long long* key0 = (unsigned long long*)take(8 * n);
  unsigned long long* key1 = (unsigned long long*)take(8 * n);
  int* val0 = (int*)take(4 * n);
  int* val1 = (int*)take(4 * n);
  int* catd = (int*)take(4 * n);
  int* hist = (int*)take(4 * 256 * tiles);
  long* seg = (long*)take(16 * (long)K);
  int* srank = (int*)take(4 * n);
  unsigned char* scode = (unsigned char*)take((long)AT * n);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  coco_sort_init_kernel<<<blocks, 256, 0, st>>>(slot_cat, slot_score, slot_rank, key0, val0, catd, n, K, max_det_host);
  auto pass = [&](int shift) {
    coco_radix_hist_kernel<<<(unsigned)tiles, kSortThreads, 0, st>>>(key0, n, shift, hist, (int)tiles);
    coco_scan_kernel<<<1, 1024, 0, st>>>(hist, 256 * tiles);
    coco_radix_scatter_kernel<<<(unsigned)tiles, kSortThreads, 0, st>>>(key0, val0, key1, val1, n, shift, hist, (int)tiles);
    unsigned long long* tk = key0; key0 = key1; key1 = tk;
    int* tv = val0; val0 = val1; val1 = tv;
  };
  for (int shift = 0; shift < 64; shift += 8) pass(shift);            // -score, least significant byte first
  coco_rekey_kernel<<<blocks, 256, 0, st>>>(val0, catd, key0, n);
  pass(0);                                                             // then the category (K = not evaluated, last)
  if (K > 255) pass(8);
  const hipError_t me = hipMemsetAsync(seg, 0, 16 * (size_t)K, st);
  if (me != hipSuccess) {
    relnet::set_error("relnet_coco_accumulate: hipMemsetAsync failed: %s", hipGetErrorString(me));
    return -1;
  }
  coco_segments_kernel<<<blocks, 256, 0, st>>>(key0, n, K, seg);
  coco_gather_kernel<<<blocks, 256, 0, st>>>(key0, val0, slot_rank, (const unsigned char*)slot_code, srank, scode, n, K, AT);
  CocoAccArgs g{seg, srank, scode, npig, rec_thr, max_dets, precision, recall, K, A, T, R, M};
  coco_accumulate_kernel<<<(unsigned)K, 64, 0, st>>>(g);
  return check_launch("relnet_coco_accumulate");
}
