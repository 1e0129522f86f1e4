// csrc/evaluate.hip -- COCO-style bbox evaluation on the device (include/lfd_hip.h, lfd_eval_*; the host side is
// lfd_amd/evaluation.py, the definition is DESIGN.md "Evaluation").  Everything is float64 and evaluated as the definition
// writes it (the library is built with -ffp-contract=off; fp64 division is correctly rounded).
//
// Stage 1, lfd_eval_match: histogram of the stored detections over the dense pair ids (image * K + category), one
// single-workgroup scan that turns it into pair offsets AND compacts the pairs that have anything to do, an atomic scatter
// of the detection indices into their pair's slots, then k_match: a persistent grid whose workgroups take one active pair
// at a time, rank its detections by (score descending, insertion index) by counting, and walk the greedy matching.  The
// T * A <= 64 matchings of a pair are independent sequential walks over the same IoU values: 256 lanes compute a
// 4-detection x 64-ground-truth IoU tile into LDS, the first T * A lanes of wave 0 walk it.  A pair with more than 64
// ground-truth boxes walks tile after tile, one detection at a time; the per-(ground truth, matching) "taken" flags are
// bytes in the workspace, so no per-pair capacity exists.
// Stage 2, lfd_eval_accumulate: LSD radix sort (8-bit digits, stable) of the pair-major list by score then category, which
// leaves every category's detections in the order the definition asks for (ties: image order, then rank); k_accumulate then
// runs one workgroup per (category, area range, max_dets entry, threshold) backwards over its category: suffix sums give
// tp / fp at every position, a suffix maximum the precision envelope, and each position that raises recall writes the
// recall points it is the first to reach.
#include "eval_store.h"

namespace {

constexpr int EV_THREADS = ES_THREADS;
constexpr int EV_SCAN_THREADS = ES_SCAN_THREADS;
constexpr int EV_GT_TILE = 64;
constexpr int EV_DPS = EV_THREADS / EV_GT_TILE;   // detections per IoU tile
constexpr int EV_RX_ITEMS = 8;
constexpr int EV_RX_TILE = EV_THREADS * EV_RX_ITEMS;
constexpr int EV_MATCH_GRID = 4096;

struct EvArgs {
  lfd_eval_bufs_t b;
  int I, K, G, cap, T, A, R, M;
  int max_dets[LFD_EVAL_MAX_MAXDETS];
  // workspace
  int* cnt;       // [P] detections per pair
  int* start;     // [P + 1]
  int* fill;      // [P]
  int* active;    // [P]
  int* members;   // [cap]
  int* cat_cnt;   // [K]
  uint8_t* gtm;   // [G, 64]
  int* perm[2];   // [cap] each
  int* ghist;     // [256 * rx_blocks]
  int rx_blocks;
};

__host__ __device__ __forceinline__ EsStore ev_store(const EvArgs& a) {
  return EsStore{a.b.det_box, a.b.det_score, a.b.det_img, a.b.det_cat, a.b.state, a.b.img_mask, a.I, a.K, a.cap};
}

struct OpMax { __device__ double operator()(double x, double y) const { return fmax(x, y); } };

// scores: -0.0 counts as 0.0, NaN as -inf (a total order, whatever the input)
__device__ __forceinline__ double ev_score(double s) {
  s = s + 0.0;
  return s == s ? s : -__builtin_huge_val();
}
// ascending key <=> descending score
__device__ __forceinline__ u64 ev_desc_key(double s) {
  const u64 u = (u64)__double_as_longlong(s);
  const u64 ord = (u >> 63) ? ~u : (u | (1ull << 63));
  return ~ord;
}

// ------------------------------------------------------------------ appends (the frame is eval_store.h)
struct EvDets : EsDetsDefaults {   // a bad ordinal: LFD_EVAL_ERR_IMAGE whether or not the entry fits, and nothing is written
  const int32_t* label_map;
  int num_labels, mark_all;
  __device__ bool marks(int c, bool fits) const { return fits && (mark_all || c > 0); }   // after the capacity test
  __device__ void row(const EsStore& s, long long o, int ord, float x1, float y1, float w, float h, float score, int lab) const {
    es_put(s, o, (double)x1, (double)y1, (double)w, (double)h, (double)score, ord);   // {x, y, w, h}, the score as is
    s.det_cat[o] = es_label_category(s, label_map, num_labels, lab);
  }
};

struct EvRows {
  static constexpr int kCols = 7;   // ordinal, category, score, x, y, w, h
  __device__ void row(const EsStore& s, long long o, const double* r, int ord, bool bad) const {
    const int cat = (int)r[1];
    es_put(s, o, r[3], r[4], r[5], r[6], r[2], bad ? 0 : ord);   // a bad ordinal: image 0 with no category
    s.det_cat[o] = (!bad && cat >= 0 && cat < s.K) ? cat : -1;   // a category out of range: -1, silently
  }
};

// ------------------------------------------------------------------ stage 1: grouping
struct EvPairKey {
  __device__ int operator()(const EsStore& s, int d) const {
    const int img = s.det_img[d], cat = s.det_cat[d];
    if (img < 0 || img >= s.I || cat < 0 || cat >= s.K || !s.img_mask[img]) return -1;
    return img * s.K + cat;
  }
};

__global__ __launch_bounds__(EV_THREADS) void k_count(EvArgs a) {
  const EsStore s = ev_store(a);
  const int n = min(a.b.state[0], a.cap);
  for (int d = blockIdx.x * EV_THREADS + threadIdx.x; d < n; d += gridDim.x * EV_THREADS) {
    const int p = EvPairKey()(s, d);
    if (p < 0) continue;
    atomicAdd(&a.cnt[p], 1);
    atomicAdd(&a.cat_cnt[p % a.K], 1);
  }
}

// one workgroup: start[] = exclusive scan of cnt[], active[] = the pairs of evaluated images that hold a detection or a
// ground-truth box, cat_start[] = exclusive scan of cat_cnt[]
__global__ __launch_bounds__(EV_SCAN_THREADS) void k_pair_scan(EvArgs a) {
  __shared__ u64 s[2 * EV_SCAN_THREADS];
  const int t = threadIdx.x;
  const long long P = (long long)a.I * a.K;
  const long long chunk = (P + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
  const long long p0 = min(P, t * chunk), p1 = min(P, p0 + chunk);
  u64 loc = 0;   // high word: active pairs, low word: detections
  for (long long p = p0; p < p1; ++p) {
    const int c = a.cnt[p];
    const bool act = a.b.img_mask[p / a.K] && (c > 0 || a.b.gt_pair_start[p + 1] > a.b.gt_pair_start[p]);
    loc += (u64)c + (act ? (1ull << 32) : 0ull);
  }
  const u64 inc = ev_block_scan<u64, EV_SCAN_THREADS>(loc, s, OpAdd());
  u64 run = inc - loc;
  for (long long p = p0; p < p1; ++p) {
    const int c = a.cnt[p];
    const bool act = a.b.img_mask[p / a.K] && (c > 0 || a.b.gt_pair_start[p + 1] > a.b.gt_pair_start[p]);
    a.start[p] = (int)(run & 0xffffffffull);
    if (act) a.active[run >> 32] = (int)p;
    run += (u64)c + (act ? (1ull << 32) : 0ull);
  }
  if (t == EV_SCAN_THREADS - 1) {
    a.start[P] = (int)(inc & 0xffffffffull);
    a.b.state[2] = (int)(inc & 0xffffffffull);
    a.b.state[3] = (int)(inc >> 32);
  }
  // categories
  const int kchunk = (a.K + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
  const int k0 = min(a.K, t * kchunk), k1 = min(a.K, k0 + kchunk);
  u64 kl = 0;
  for (int k = k0; k < k1; ++k) kl += (u64)a.cat_cnt[k];
  const u64 kinc = ev_block_scan<u64, EV_SCAN_THREADS>(kl, s, OpAdd());
  u64 krun = kinc - kl;
  for (int k = k0; k < k1; ++k) {
    a.b.cat_start[k] = (int)krun;
    krun += (u64)a.cat_cnt[k];
  }
  if (t == EV_SCAN_THREADS - 1) a.b.cat_start[a.K] = (int)kinc;
}

// ------------------------------------------------------------------ stage 1: rank + match
__global__ __launch_bounds__(EV_THREADS) void k_match(EvArgs a) {
  __shared__ double s_sc[EV_THREADS];
  __shared__ int s_ix[EV_THREADS];
  __shared__ double s_iou[EV_DPS][EV_GT_TILE];
  __shared__ double s_gar[EV_GT_TILE];
  __shared__ int s_gcr[EV_GT_TILE];
  const int tid = threadIdx.x;
  const int n_active = a.b.state[3];
  const int TA = a.T * a.A;
  const int max_last = a.max_dets[a.M - 1];
  double thr = 0.0, lo = 0.0, hi = 0.0;
  if (tid < TA) {
    thr = fmin(a.b.iou_thrs[tid / a.A], 1.0 - 1e-10);
    lo = a.b.area_rng[2 * (tid % a.A)];
    hi = a.b.area_rng[2 * (tid % a.A) + 1];
  }
  for (int w = blockIdx.x; w < n_active; w += gridDim.x) {
    const int p = a.active[w];
    const int k = p % a.K;
    const int d0 = a.start[p], nd = a.start[p + 1] - d0;
    const int g0 = a.b.gt_pair_start[p], ng = a.b.gt_pair_start[p + 1] - g0;

    // rank by counting: position = number of detections of the pair that come before this one
    for (int ib = 0; ib < nd; ib += EV_THREADS) {
      const int i = ib + tid;
      const bool valid = i < nd;
      int my = -1;
      double ms = 0.0;
      if (valid) {
        my = a.members[d0 + i];
        ms = ev_score(a.b.det_score[my]);
      }
      int r = 0;
      for (int jb = 0; jb < nd; jb += EV_THREADS) {
        __syncthreads();
        if (jb + tid < nd) {
          const int o = a.members[d0 + jb + tid];
          s_ix[tid] = o;
          s_sc[tid] = ev_score(a.b.det_score[o]);
        }
        __syncthreads();
        if (valid) {
          const int lim = min(EV_THREADS, nd - jb);
          for (int jj = 0; jj < lim; ++jj) {
            const double sj = s_sc[jj];
            r += (sj > ms || (sj == ms && s_ix[jj] < my)) ? 1 : 0;
          }
        }
      }
      if (valid) {
        const int s = d0 + r;
        a.b.order[s] = my;
        a.b.sort_key[s] = ev_desc_key(ms);
        a.b.sorted_cat[s] = k;
        a.b.sorted_rank[s] = r;
        a.b.match_bits[s] = 0ull;
        a.b.ignore_bits[s] = 0ull;
      }
    }
    // this pair's "taken" flags, and its share of the non-ignored ground truth
    {
      u64* gz = reinterpret_cast<u64*>(a.gtm + (size_t)g0 * 64);
      for (int x = tid; x < ng * 8; x += EV_THREADS) gz[x] = 0ull;
      if (tid < a.A) {
        const double alo = a.b.area_rng[2 * tid], ahi = a.b.area_rng[2 * tid + 1];
        int c = 0;
        for (int g = 0; g < ng; ++g) {
          const double ar = a.b.gt_area[g0 + g];
          c += (!a.b.gt_crowd[g0 + g] && !(ar < alo || ar > ahi)) ? 1 : 0;
        }
        if (c) atomicAdd(&a.b.npig[k * a.A + tid], c);
      }
    }
    __syncthreads();

    const int ndm = min(nd, max_last);
    const int dps = ng <= EV_GT_TILE ? EV_DPS : 1;
    for (int db = 0; db < ndm; db += dps) {
      double b1 = thr, b2 = thr;   // best IoU among the non-ignored / the ignored ground truth
      int m1 = -1, m2 = -1;
      for (int gb = 0; gb == 0 || gb < ng; gb += EV_GT_TILE) {
        __syncthreads();
        {
          const int dq = tid / EV_GT_TILE, gj = tid % EV_GT_TILE;
          const int d = db + dq, g = gb + gj;
          if (g < ng) {
            const int crowd = a.b.gt_crowd[g0 + g];
            if (dq == 0) {
              s_gar[gj] = a.b.gt_area[g0 + g];
              s_gcr[gj] = crowd;
            }
            if (dq < dps && d < ndm) {
              const double* bd = a.b.det_box + (size_t)a.b.order[d0 + d] * 4;
              const double* bg = a.b.gt_box + (size_t)(g0 + g) * 4;
              const double dx = bd[0], dy = bd[1], dw = bd[2], dh = bd[3];
              const double gx = bg[0], gy = bg[1], gw = bg[2], gh = bg[3];
              const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
              const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
              double iou = 0.0;
              if (iw > 0.0 && ih > 0.0) {
                const double inter = iw * ih;
                const double uni = crowd ? dw * dh : dw * dh + gw * gh - inter;
                iou = inter / uni;
              }
              s_iou[dq][gj] = iou;
            }
          }
        }
        __syncthreads();
        if (tid < TA) {
          const int lim = max(0, min(EV_GT_TILE, ng - gb));
          for (int dq = 0; dq < dps && db + dq < ndm; ++dq) {
            if (dps > 1) {
              b1 = b2 = thr;
              m1 = m2 = -1;
            }
            for (int gj = 0; gj < lim; ++gj) {
              const double iou = s_iou[dq][gj];
              const int crowd = s_gcr[gj];
              const double ar = s_gar[gj];
              const bool ig = crowd || ar < lo || ar > hi;
              if (iou < (ig ? b2 : b1)) continue;
              if (!crowd && a.gtm[(size_t)(g0 + gb + gj) * 64 + tid]) continue;
              if (ig) {
                b2 = iou;
                m2 = gb + gj;
              } else {
                b1 = iou;
                m1 = gb + gj;
              }
            }
            if (dps > 1 || gb + EV_GT_TILE >= ng) {   // the detection has seen all its ground truth
              const int m = m1 >= 0 ? m1 : m2;
              const bool matched = m >= 0;
              bool ig;
              if (matched) {
                const size_t gi = (size_t)g0 + m;
                a.gtm[gi * 64 + tid] = 1;
                const double ar = a.b.gt_area[gi];
                ig = a.b.gt_crowd[gi] || ar < lo || ar > hi;
              } else {
                const double* bd = a.b.det_box + (size_t)a.b.order[d0 + db + dq] * 4;
                const double darea = bd[2] * bd[3];
                ig = darea < lo || darea > hi;
              }
              const u64 mb = __ballot(matched), ib = __ballot(ig);
              if (tid == 0) {
                a.b.match_bits[d0 + db + dq] = mb;
                a.b.ignore_bits[d0 + db + dq] = ib;
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ stage 2: radix sort of the pair-major list
__device__ __forceinline__ int ev_digit(const EvArgs& a, int s, int pass) {
  return pass < 8 ? (int)((a.b.sort_key[s] >> (8 * pass)) & 0xff) : (a.b.sorted_cat[s] >> (8 * (pass - 8))) & 0xff;
}

__global__ __launch_bounds__(EV_THREADS) void k_rx_init(EvArgs a) {
  const int n = min(a.b.state[2], a.cap);
  for (int i = blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += gridDim.x * EV_THREADS) a.perm[0][i] = i;
}

__global__ __launch_bounds__(EV_THREADS) void k_rx_hist(EvArgs a, int pass, int src) {
  __shared__ int s_h[256];
  const int tid = threadIdx.x;
  s_h[tid] = 0;
  __syncthreads();
  const int n = min(a.b.state[2], a.cap);
  const int base = blockIdx.x * EV_RX_TILE;
  for (int it = 0; it < EV_RX_ITEMS; ++it) {
    const int i = base + it * EV_THREADS + tid;
    if (i < n) atomicAdd(&s_h[ev_digit(a, a.perm[src][i], pass)], 1);
  }
  __syncthreads();
  a.ghist[tid * a.rx_blocks + blockIdx.x] = s_h[tid];
}

// exclusive scan, in place, of data[0 .. L) by one workgroup
__global__ __launch_bounds__(EV_SCAN_THREADS) void k_excl_scan(int* data, int L) {
  __shared__ u64 s[2 * EV_SCAN_THREADS];
  const int t = threadIdx.x;
  const int chunk = (L + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
  const int i0 = min(L, t * chunk), i1 = min(L, i0 + chunk);
  u64 loc = 0;
  for (int i = i0; i < i1; ++i) loc += (u64)data[i];
  const u64 inc = ev_block_scan<u64, EV_SCAN_THREADS>(loc, s, OpAdd());
  u64 run = inc - loc;
  for (int i = i0; i < i1; ++i) {
    const int v = data[i];
    data[i] = (int)run;
    run += (u64)v;
  }
}

__global__ __launch_bounds__(EV_THREADS) void k_rx_scatter(EvArgs a, int pass, int src) {
  __shared__ int s_base[256];
  __shared__ int s_wcnt[EV_THREADS / 64][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_base[tid] = a.ghist[tid * a.rx_blocks + blockIdx.x];
  const int n = min(a.b.state[2], a.cap);
  const int base = blockIdx.x * EV_RX_TILE;
  const int* in = a.perm[src];
  int* out = a.perm[src ^ 1];
  for (int it = 0; it < EV_RX_ITEMS; ++it) {
    for (int x = tid; x < (EV_THREADS / 64) * 256; x += EV_THREADS) (&s_wcnt[0][0])[x] = 0;
    __syncthreads();
    const int i = base + it * EV_THREADS + tid;
    const bool valid = i < n;
    int val = 0, dg = 0;
    if (valid) {
      val = in[i];
      dg = ev_digit(a, val, pass);
    }
    // lanes of this wave that hold the same digit
    u64 same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (dg >> bit) & 1;
      const u64 bal = __ballot(valid && one);
      same &= one ? bal : ~bal;
    }
    const int lrank = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && lrank == 0) s_wcnt[wave][dg] = __popcll(same);
    __syncthreads();
    if (valid) {
      int off = s_base[dg] + lrank;
      for (int w = 0; w < wave; ++w) off += s_wcnt[w][dg];
      if (off >= 0 && off < a.cap) out[off] = val;
    }
    __syncthreads();
    {
      int add = 0;
      for (int w = 0; w < EV_THREADS / 64; ++w) add += s_wcnt[w][tid];
      s_base[tid] += add;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ stage 2: precision / recall
__global__ __launch_bounds__(EV_THREADS) void k_accumulate(EvArgs a, int src) {
  __shared__ u64 s_sum[2 * EV_THREADS];
  __shared__ double s_max[2 * EV_THREADS];
  __shared__ double s_q[LFD_EVAL_MAX_RECTHRS];
  __shared__ double s_rec[LFD_EVAL_MAX_RECTHRS];
  __shared__ u64 s_carry;
  __shared__ double s_cmax;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % a.T;
  b /= a.T;
  const int m = b % a.M;
  b /= a.M;
  const int ar = b % a.A;
  const int k = b / a.A;
  const int npig = a.b.npig[k * a.A + ar];
  double* rec_out = a.b.recall + (((size_t)t * a.K + k) * a.A + ar) * a.M + m;
  // precision[t, r, k, ar, m]
  const size_t p_first = (((size_t)t * a.R * a.K + k) * a.A + ar) * a.M + m;
  const size_t p_step = (size_t)a.K * a.A * a.M;
  if (npig == 0) {
    for (int r = tid; r < a.R; r += EV_THREADS) a.b.precision[p_first + r * p_step] = -1.0;
    if (tid == 0) *rec_out = -1.0;
    return;
  }
  for (int r = tid; r < a.R; r += EV_THREADS) {
    s_q[r] = 0.0;
    s_rec[r] = a.b.rec_thrs[r];
  }
  const int c0 = a.b.cat_start[k], n = a.b.cat_start[k + 1] - c0;
  const int md = a.max_dets[m];
  const int bit = t * a.A + ar;
  const int* perm = a.perm[src];
  // increments of position j: true positive in the high word, false positive in the low word
  auto inc_of = [&](int j) -> u64 {
    const int s = perm[c0 + j];
    if (a.b.sorted_rank[s] >= md || ((a.b.ignore_bits[s] >> bit) & 1ull)) return 0ull;
    return ((a.b.match_bits[s] >> bit) & 1ull) ? (1ull << 32) : 1ull;
  };
  u64 loc = 0;
  for (int j = tid; j < n; j += EV_THREADS) loc += inc_of(j);
  const u64 tot_inc = ev_block_scan<u64, EV_THREADS>(loc, s_sum, OpAdd());
  if (tid == EV_THREADS - 1) s_carry = tot_inc;
  __syncthreads();
  const u64 tot = s_carry;
  __syncthreads();
  const long long tp_tot = (long long)(tot >> 32), fp_tot = (long long)(tot & 0xffffffffull);
  const double eps = 2.220446049250313e-16;   // np.spacing(1)
  const double dn = (double)npig;
  u64 carry = 0;
  double cmax = 0.0;
  for (int qb = 0; qb < n; qb += EV_THREADS) {   // backwards: q counts from the last position
    const int q = qb + tid;
    const bool valid = q < n;
    const int j = n - 1 - q;
    const u64 v = valid ? inc_of(j) : 0ull;
    const u64 S = ev_block_scan<u64, EV_THREADS>(v, s_sum, OpAdd()) + carry;   // increments of positions >= j
    const long long v_tp = (long long)(v >> 32), v_fp = (long long)(v & 0xffffffffull);
    const long long tp = tp_tot - ((long long)(S >> 32) - v_tp);
    const long long fp = fp_tot - ((long long)(S & 0xffffffffull) - v_fp);
    const double pr = valid ? (double)tp / ((double)fp + (double)tp + eps) : 0.0;
    const double env = fmax(ev_block_scan<double, EV_THREADS>(pr, s_max, OpMax()), cmax);
    if (valid && (v_tp || j == 0)) {
      const double rcj = (double)tp / dn, rcp = (double)(tp - v_tp) / dn;
      for (int r = 0; r < a.R; ++r) {
        const double rt = s_rec[r];
        if (rcj >= rt && !(j > 0 && rcp >= rt)) s_q[r] = env;
      }
    }
    if (tid == EV_THREADS - 1) {
      s_carry = S;
      s_cmax = env;
    }
    __syncthreads();
    carry = s_carry;
    cmax = s_cmax;
    __syncthreads();
  }
  __syncthreads();
  for (int r = tid; r < a.R; r += EV_THREADS) a.b.precision[p_first + r * p_step] = s_q[r];
  if (tid == 0) *rec_out = (double)tp_tot / dn;
}

// ------------------------------------------------------------------ host
bool ev_desc_ok(const lfd_eval_desc_t* d) {
  if (!d) return false;
  if (d->num_images < 1 || d->num_categories < 1 || d->num_gt < 0 || d->det_capacity < 1) return false;
  if (d->num_iou_thrs < 1 || d->num_area_rngs < 1 || d->num_iou_thrs * (long long)d->num_area_rngs > 64) return false;
  if (d->num_rec_thrs < 1 || d->num_rec_thrs > LFD_EVAL_MAX_RECTHRS) return false;
  if (d->num_max_dets < 1 || d->num_max_dets > LFD_EVAL_MAX_MAXDETS) return false;
  for (int i = 0; i < d->num_max_dets; ++i)
    if (d->max_dets[i] < 1 || (i && d->max_dets[i] < d->max_dets[i - 1])) return false;
  return true;
}
// the dense pair table and the packed counters of the scans are 32-bit
bool ev_desc_supported(const lfd_eval_desc_t* d) {
  return (long long)d->num_images * d->num_categories <= (1LL << 28) && d->num_categories <= 65536 &&
         d->det_capacity <= (1 << 30) && d->num_gt <= (1 << 24);
}

int ev_rx_blocks(const lfd_eval_desc_t* d) { return (d->det_capacity + EV_RX_TILE - 1) / EV_RX_TILE; }

EvArgs ev_args(const lfd_eval_desc_t* d, const lfd_eval_bufs_t* b) {
  EvArgs a{};
  if (b) a.b = *b;
  a.I = d->num_images; a.K = d->num_categories; a.G = d->num_gt; a.cap = d->det_capacity;
  a.T = d->num_iou_thrs; a.A = d->num_area_rngs; a.R = d->num_rec_thrs; a.M = d->num_max_dets;
  for (int i = 0; i < LFD_EVAL_MAX_MAXDETS; ++i) a.max_dets[i] = i < a.M ? d->max_dets[i] : 0;
  a.rx_blocks = ev_rx_blocks(d);
  return a;
}

size_t ev_carve_match(EvArgs& a, void* ws) {
  LfdCarver c(ws);
  const size_t P = (size_t)a.I * a.K;
  // cnt, fill, cat_cnt are contiguous: one memset zeroes them
  a.cnt = c.take<int>(2 * P + a.K);
  a.fill = a.cnt + P;
  a.cat_cnt = a.fill + P;
  a.start = c.take<int>(P + 1);
  a.active = c.take<int>(P);
  a.members = c.take<int>(a.cap);
  a.gtm = c.take<uint8_t>((size_t)max(a.G, 1) * 64);
  return c.used();
}

size_t ev_carve_acc(EvArgs& a, void* ws) {
  LfdCarver c(ws);
  a.perm[0] = c.take<int>(a.cap);
  a.perm[1] = c.take<int>(a.cap);
  a.ghist = c.take<int>((size_t)256 * a.rx_blocks);
  return c.used();
}

bool ev_store_ok(const lfd_eval_bufs_t* b) {
  return b && b->det_box && b->det_score && b->det_img && b->det_cat && b->state && b->img_mask;
}

}  // namespace

extern "C" {

int lfd_eval_append_dets_f32(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, const float* dets, const int32_t* labels,
                             const int32_t* counts, int32_t n, int32_t cap, const int32_t* label_map, int32_t num_labels,
                             const int32_t* img_ord, int32_t mark_all, lfd_stream_t stream) {
  if (!ev_desc_ok(desc) || !ev_store_ok(bufs) || !dets || !labels || !counts || !label_map || !img_ord) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || cap < 1 || num_labels < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!ev_desc_supported(desc) || n > 65535) return LFD_ERR_UNSUPPORTED;
  EvDets p;
  p.label_map = label_map;
  p.num_labels = num_labels;
  p.mark_all = mark_all;
  return es_append_dets(ev_store(ev_args(desc, bufs)), p, dets, labels, counts, n, cap, img_ord, 0, stream);
}

int lfd_eval_append_rows_f64(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, const double* rows, int64_t m,
                             const int32_t* mark, int32_t num_mark, lfd_stream_t stream) {
  if (!ev_desc_ok(desc) || !ev_store_ok(bufs) || m < 0 || num_mark < 0) return LFD_ERR_INVALID_ARGUMENT;
  if ((m > 0 && !rows) || (num_mark > 0 && !mark)) return LFD_ERR_INVALID_ARGUMENT;
  if (!ev_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  if (m == 0 && num_mark == 0) return LFD_OK;
  return es_append_rows(ev_store(ev_args(desc, bufs)), EvRows(), rows, (long long)m, mark, num_mark, stream);
}

size_t lfd_eval_match_workspace_bytes(const lfd_eval_desc_t* desc) {
  if (!ev_desc_ok(desc) || !ev_desc_supported(desc)) return 0;
  EvArgs a = ev_args(desc, nullptr);
  return ev_carve_match(a, nullptr);
}

int lfd_eval_match(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, void* workspace, size_t workspace_bytes,
                   lfd_stream_t stream) {
  if (!ev_desc_ok(desc) || !ev_store_ok(bufs) || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (!bufs->gt_pair_start || !bufs->iou_thrs || !bufs->area_rng || !bufs->order || !bufs->sort_key || !bufs->sorted_cat ||
      !bufs->sorted_rank || !bufs->match_bits || !bufs->ignore_bits || !bufs->npig || !bufs->cat_start)
    return LFD_ERR_INVALID_ARGUMENT;
  if (desc->num_gt > 0 && (!bufs->gt_box || !bufs->gt_area || !bufs->gt_crowd)) return LFD_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return LFD_ERR_INVALID_ARGUMENT;
  if (!ev_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  EvArgs a = ev_args(desc, bufs);
  if (ev_carve_match(a, workspace) > workspace_bytes) return LFD_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t P = (size_t)a.I * a.K;
  if (hipMemsetAsync(a.cnt, 0, (2 * P + a.K) * sizeof(int), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (hipMemsetAsync(a.b.npig, 0, (size_t)a.K * a.A * sizeof(int), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  hipLaunchKernelGGL(k_count, dim3(es_grid(a.cap)), dim3(EV_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_pair_scan, dim3(1), dim3(EV_SCAN_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_scatter<EvPairKey>, dim3(es_grid(a.cap)), dim3(EV_THREADS), 0, st, ev_store(a), a.start, a.fill, a.members);
  LFD_CHECK_LAUNCH();
  const long long pairs_max = min((long long)P, (long long)a.cap + a.G);
  hipLaunchKernelGGL(k_match, dim3((unsigned)max(1LL, min(pairs_max, (long long)EV_MATCH_GRID))), dim3(EV_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

size_t lfd_eval_accumulate_workspace_bytes(const lfd_eval_desc_t* desc) {
  if (!ev_desc_ok(desc) || !ev_desc_supported(desc)) return 0;
  EvArgs a = ev_args(desc, nullptr);
  return ev_carve_acc(a, nullptr);
}

int lfd_eval_accumulate(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, void* workspace, size_t workspace_bytes,
                        lfd_stream_t stream) {
  if (!ev_desc_ok(desc) || !bufs || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (!bufs->state || !bufs->rec_thrs || !bufs->sort_key || !bufs->sorted_cat || !bufs->sorted_rank || !bufs->match_bits ||
      !bufs->ignore_bits || !bufs->npig || !bufs->cat_start || !bufs->precision || !bufs->recall)
    return LFD_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return LFD_ERR_INVALID_ARGUMENT;
  if (!ev_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  EvArgs a = ev_args(desc, bufs);
  if (ev_carve_acc(a, workspace) > workspace_bytes) return LFD_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_rx_init, dim3(es_grid(a.cap)), dim3(EV_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  // 8 passes over the score key, then the category index (nothing to sort by with one category)
  const int cat_passes = a.K <= 1 ? 0 : (a.K <= 256 ? 1 : 2);
  int src = 0;
  for (int pass = 0; pass < 8 + cat_passes; ++pass) {
    hipLaunchKernelGGL(k_rx_hist, dim3(a.rx_blocks), dim3(EV_THREADS), 0, st, a, pass, src);
    LFD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_excl_scan, dim3(1), dim3(EV_SCAN_THREADS), 0, st, a.ghist, 256 * a.rx_blocks);
    LFD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rx_scatter, dim3(a.rx_blocks), dim3(EV_THREADS), 0, st, a, pass, src);
    LFD_CHECK_LAUNCH();
    src ^= 1;
  }
  const long long cells = (long long)a.K * a.A * a.M * a.T;
  if (cells >= (1LL << 31)) return LFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_accumulate, dim3((unsigned)cells), dim3(EV_THREADS), 0, st, a, src);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
