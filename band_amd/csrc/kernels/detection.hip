// TFLite_Detection_PostProcess on the device (bh_detection_postprocess):
// the restatement of CpuDetectionPostprocess (backend/hip/cpu_kernels.cc) -
// fast class-agnostic NMS, one class per detection - as two kernels with no
// host step between them, so a pass is capturable and replayable.
//
// This file is compiled with -ffp-contract=off (Makefile): the box decode
// (double) and the IoU (float) round every operation separately, as the
// host code and the reference do.
//
// Scratch (bh_detection_scratch_bytes), per call, for B = batch * num_boxes:
//   keys  [B] u64   candidate key per anchor (det_key.hpp), 0 = not a candidate
//   ckeys [B] u64   an image's candidates compacted in anchor order; 0 = inactive
//   cbox  [B] f32x4 their decoded boxes (ymin xmin ymax xmax)
//   cls   [B] i32   per anchor, the class of its maximum
// detection_score_kernel writes every keys / cls entry; detection_nms_kernel
// writes the first `candidates` entries of ckeys / cbox before it reads them
// and never reads beyond, so nothing of an earlier call is ever seen.
// Nothing depends on the order of atomics: there are none.
#include "common.hpp"
#include "det_key.hpp"

namespace bh {

constexpr int kDetScoreThreads = 256;
constexpr int kDetNmsThreads = 1024;
constexpr int kDetNmsWaves = kDetNmsThreads / kWave;

struct DetScratch {
  unsigned long long* keys;
  unsigned long long* ckeys;
  float4* cbox;
  int* cls;
};

__host__ __device__ inline DetScratch det_scratch(void* base, long total) {
  DetScratch s;
  s.keys = (unsigned long long*)base;
  s.ckeys = s.keys + total;
  s.cbox = (float4*)(s.ckeys + total);
  s.cls = (int*)(s.cbox + total);
  return s;
}

// DEQUANTIZE of one byte, the value of the glue lowering's table
// (quant.cc DequantizeTable: float(double(scale) * double(q - zp))): the
// double product of a float and a 9-bit integer is exact, so rounding it to
// float is the correctly rounded float product, which is this multiply
__device__ __forceinline__ float det_dequant(float scale, int q, int zp) { return scale * (float)(q - zp); }

// Score pass.  L lanes share an anchor's row (contiguous, 1 or 4 bytes per
// class): lane l scans classes l, l + L, .. upwards with a strict `>` (its
// first maximum), then an xor butterfly over the L lanes merges on (value
// descending, class ascending) - the row's first maximum.  TYPE 0: float
// scores, where the sequential scan `mx = row[0]; if (row[c] > mx)` never
// takes a NaN after class 0 and stays NaN when row[0] is one; TYPE 1 / 2:
// int8 / uint8 bytes compared as integers (dequantisation is strictly
// increasing for scale > 0, so byte ties are exactly float ties) and only
// the maximum is dequantised.
template <int L, int TYPE>
__global__ __launch_bounds__(kDetScoreThreads) void detection_score_kernel(bh_detection_params p, long total) {
  const long g = ((long)blockIdx.x * kDetScoreThreads + threadIdx.x) / L;
  const int l = threadIdx.x % L;
  const bool live = g < total;  // (dead lanes still take part in the shuffles)
  const int cwb = p.num_classes_with_background;
  const int nc = p.num_classes;
  const long row = g * cwb + (cwb - nc);
  bool have = false;
  int arg = 0;
  bool nan0 = false;
  float vf = 0.f;
  int vi = 0;
  if (live) {
    if (TYPE == 0) {
      const float* x = (const float*)p.class_scores + row;
      for (int c = l; c < nc; c += L) {
        const float v = x[c];
        if (v != v) {
          nan0 = nan0 || c == 0;
          continue;
        }
        if (!have || v > vf) {
          vf = v;
          arg = c;
          have = true;
        }
      }
    } else {
      const unsigned char* x = (const unsigned char*)p.class_scores + row;
      for (int c = l; c < nc; c += L) {
        const int v = TYPE == 1 ? (int)(signed char)x[c] : (int)x[c];
        if (!have || v > vi) {
          vi = v;
          arg = c;
          have = true;
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < L; m <<= 1) {
    const int h2 = __shfl_xor((int)have, m, L);
    const int a2 = __shfl_xor(arg, m, L);
    bool take;
    if (TYPE == 0) {
      const float v2 = __shfl_xor(vf, m, L);
      take = h2 && (!have || v2 > vf || (v2 == vf && a2 < arg));
      if (take) vf = v2;
    } else {
      const int v2 = __shfl_xor(vi, m, L);
      take = h2 && (!have || v2 > vi || (v2 == vi && a2 < arg));
      if (take) vi = v2;
    }
    if (take) {
      arg = a2;
      have = true;
    }
  }
  if (!live || l != 0) return;
  const DetScratch s = det_scratch(p.scratch, total);
  const float score = TYPE == 0 ? vf : det_dequant(p.score_scale, vi, p.score_zp);
  // row[0] NaN (lane 0 reads class 0): the maximum is NaN, never a candidate
  const bool cand = have && !nan0 && score >= p.score_threshold;
  const unsigned i = (unsigned)(g % p.num_boxes);
  s.keys[g] = cand ? bh_det_key(score, i) : 0ull;
  s.cls[g] = have && !nan0 ? arg : 0;
}

// DecodeCenterSizeBoxes for one anchor, in the operation order of
// CpuDetectionPostprocess: double arithmetic, rounded to float, corners in float
template <int TYPE>
__device__ __forceinline__ float4 det_decode(const bh_detection_params& p, long g, int i) {
  float be[4];
  if (TYPE == 0) {
    const float4 v = ((const float4*)p.box_encodings)[g];
    be[0] = v.x; be[1] = v.y; be[2] = v.z; be[3] = v.w;
  } else {
    const unsigned w = ((const unsigned*)p.box_encodings)[g];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = TYPE == 1 ? (int)(signed char)((w >> (8 * k)) & 0xffu) : (int)((w >> (8 * k)) & 0xffu);
      be[k] = det_dequant(p.box_scale, q, p.box_zp);
    }
  }
  const float4 an = ((const float4*)p.anchors)[i];  // ycenter xcenter h w
  const float yc = (float)((double)be[0] / (double)p.scale_y * (double)an.z + (double)an.x);
  const float xc = (float)((double)be[1] / (double)p.scale_x * (double)an.w + (double)an.y);
  const float hh = (float)(0.5 * exp((double)be[2] / (double)p.scale_h) * (double)an.z);
  const float hw = (float)(0.5 * exp((double)be[3] / (double)p.scale_w) * (double)an.w);
  return make_float4(yc - hh, xc - hw, yc + hh, xc + hw);
}

__device__ __forceinline__ float det_area(const float4& b) { return (b.z - b.x) * (b.w - b.y); }

// IoU of the selected box `s` against candidate `c`: the float expression of
// CpuDetectionPostprocess (std::max / std::min spelled out)
__device__ __forceinline__ float det_iou(const float4& s, float as, const float4& c) {
  const float ac = det_area(c);
  float iou = 0.0f;
  if (as > 0.0f && ac > 0.0f) {
    const float iy0 = s.x < c.x ? c.x : s.x, ix0 = s.y < c.y ? c.y : s.y;
    const float iy1 = c.z < s.z ? c.z : s.z, ix1 = c.w < s.w ? c.w : s.w;
    const float dy = iy1 - iy0, dx = ix1 - ix0;
    const float inter = (dy < 0.0f ? 0.0f : dy) * (dx < 0.0f ? 0.0f : dx);
    iou = __fdiv_rn(inter, as + ac - inter);
  }
  return iou;
}

__device__ __forceinline__ unsigned long long det_wave_max(unsigned long long v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// One workgroup per image.  (a) compaction: the image's candidates, in anchor
// order, into ckeys (each wave a contiguous run of anchors: ballot prefix
// inside the wave, per-wave counts through LDS; order-preserving and
// deterministic, one barrier).  Thread t then owns entries t, t + 1024, ..
// for the rest of the kernel: it decodes their boxes into cbox (candidates
// only, and densely - the double exp is the expensive part) and alone
// writes and re-reads them.  (b) rounds: the largest active
// key of the workgroup is the next selection (the reference's stable
// descending order: only selected boxes suppress, so the first candidate in
// that order that is still active is exactly the next box the reference's
// sweep selects); its owner emits it; every thread then clears those of its
// active entries whose IoU with it exceeds the threshold and finds its next
// local maximum in the same sweep.
template <int BT>
__global__ __launch_bounds__(kDetNmsThreads) void detection_nms_kernel(bh_detection_params p) {
  __shared__ int wave_cnt[kDetNmsWaves];
  __shared__ unsigned long long wave_max[kDetNmsWaves];
  __shared__ float sel_box[4];
  const int img = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  const int n = p.num_boxes;
  const long total = (long)p.batch * n;
  const long g0 = (long)img * n;
  const DetScratch s = det_scratch(p.scratch, total);
  const unsigned long long* keys = s.keys + g0;
  unsigned long long* ckeys = s.ckeys + g0;
  float4* cbox = s.cbox + g0;
  const int* cls = s.cls + g0;
  const int D = p.max_detections;
  float* out_boxes = p.out_boxes + (long)img * D * 4;
  float* out_classes = p.out_classes + (long)img * D;
  float* out_scores = p.out_scores + (long)img * D;

  // wave w compacts the contiguous anchors [w0, w1) (a multiple of 64 per
  // wave): it counts its candidates, learns where its run starts from the
  // waves before it, then writes them in anchor order
  const int per_wave = ((n + kDetNmsWaves - 1) / kDetNmsWaves + kWave - 1) / kWave * kWave;
  const int w0 = w * per_wave;
  const int w1 = n < w0 + per_wave ? n : w0 + per_wave;
  int cnt = 0;
  for (int i0 = w0; i0 < w1; i0 += kWave) {
    const int i = i0 + lane;
    cnt += __popcll(__ballot(i < w1 && keys[i] != 0ull));
  }
  if (lane == 0) wave_cnt[w] = cnt;
  __syncthreads();
  int pos = 0, m = 0;  // this wave's next slot; the image's candidates
#pragma unroll
  for (int j = 0; j < kDetNmsWaves; ++j) {
    const int c = wave_cnt[j];
    pos += j < w ? c : 0;
    m += c;
  }
  for (int i0 = w0; i0 < w1; i0 += kWave) {
    const int i = i0 + lane;
    const unsigned long long k = i < w1 ? keys[i] : 0ull;
    const unsigned long long ball = __ballot(k != 0ull);
    if (k != 0ull) ckeys[pos + __popcll(ball & ((1ull << lane) - 1ull))] = k;
    pos += __popcll(ball);
  }
  __syncthreads();  // ckeys visible to their owners

  // the owner decodes its candidates' boxes (dense: every lane has work) and
  // finds its first local maximum
  unsigned long long lmax = 0ull;
  int lpos = -1;
  for (int e = tid; e < m; e += kDetNmsThreads) {
    const unsigned long long k = ckeys[e];
    const int i = (int)bh_det_key_index(k);
    cbox[e] = det_decode<BT>(p, g0 + i, i);
    if (k > lmax) {
      lmax = k;
      lpos = e;
    }
  }
  const int out_size = m < D ? m : D;
  int selected = 0;
  while (selected < out_size) {
    const unsigned long long wm = det_wave_max(lmax);
    if (lane == 0) wave_max[w] = wm;
    __syncthreads();
    unsigned long long gmax = 0ull;
#pragma unroll
    for (int j = 0; j < kDetNmsWaves; ++j) {
      const unsigned long long v = wave_max[j];
      gmax = v > gmax ? v : gmax;
    }
    if (gmax == 0ull) break;  // every candidate selected or suppressed (uniform)
    if (lmax == gmax) {       // keys are unique (the anchor index): one owner
      const float4 b = cbox[lpos];
      sel_box[0] = b.x; sel_box[1] = b.y; sel_box[2] = b.z; sel_box[3] = b.w;
      out_boxes[4 * selected] = b.x;
      out_boxes[4 * selected + 1] = b.y;
      out_boxes[4 * selected + 2] = b.z;
      out_boxes[4 * selected + 3] = b.w;
      out_classes[selected] = (float)cls[bh_det_key_index(gmax)];
      out_scores[selected] = bh_det_key_score(gmax);
      ckeys[lpos] = 0ull;
    }
    __syncthreads();  // sel_box written; wave_max read by everyone
    ++selected;
    if (selected == out_size) break;
    const float4 sb = make_float4(sel_box[0], sel_box[1], sel_box[2], sel_box[3]);
    const float as = det_area(sb);
    lmax = 0ull;
    lpos = -1;
    for (int e = tid; e < m; e += kDetNmsThreads) {
      const unsigned long long k = ckeys[e];
      if (k == 0ull) continue;
      if (det_iou(sb, as, cbox[e]) > p.iou_threshold) {
        ckeys[e] = 0ull;
      } else if (k > lmax) {
        lmax = k;
        lpos = e;
      }
    }
    // sel_box / wave_max are next written after the next round's first
    // barrier / by lanes that have passed this round's second one
  }
  for (int r = selected + tid; r < D; r += kDetNmsThreads) {
    out_boxes[4 * r] = 0.f;
    out_boxes[4 * r + 1] = 0.f;
    out_boxes[4 * r + 2] = 0.f;
    out_boxes[4 * r + 3] = 0.f;
    out_classes[r] = 0.f;
    out_scores[r] = 0.f;
  }
  if (tid == 0) p.out_num[img] = (float)selected;
}

}  // namespace bh

extern "C" size_t bh_detection_scratch_bytes(int batch, int num_boxes) {
  if (batch <= 0 || num_boxes <= 0) return 0;
  return (size_t)batch * (size_t)num_boxes * (8 + 8 + 16 + 4);
}

extern "C" int bh_detection_postprocess(const bh_detection_params* pp, bh_stream_t stream) {
  if (!pp || pp->num_boxes <= 0 || pp->batch <= 0 || pp->num_classes <= 0 ||
      pp->num_classes > pp->num_classes_with_background || pp->max_detections <= 0 || !pp->box_encodings ||
      !pp->class_scores || !pp->anchors || !pp->out_boxes || !pp->out_classes || !pp->out_scores || !pp->out_num ||
      !pp->scratch || pp->box_type < 0 || pp->box_type > 2 || pp->score_type < 0 || pp->score_type > 2 ||
      (pp->score_type != 0 && !(pp->score_scale > 0.0f))) {
    bh_set_last_error("bh_detection_postprocess: invalid parameters");
    return BH_EINVAL;
  }
  const bh_detection_params& p = *pp;
  const long total = (long)p.batch * p.num_boxes;
  if (total >= INT32_MAX / 16 || (long)p.batch * p.max_detections >= INT32_MAX / 4) {
    bh_set_last_error("bh_detection_postprocess: too many boxes for 32-bit indexing");
    return BH_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  // few classes: 4 lanes per anchor; a detector's 90 / 91: 16 (64-byte runs
  // of a float row per load instruction)
  const bool wide = p.num_classes > 16;
  const int lanes = wide ? 16 : 4;
  const dim3 grid((unsigned)((total * lanes + bh::kDetScoreThreads - 1) / bh::kDetScoreThreads));
  const dim3 block(bh::kDetScoreThreads);
#define BH_DET_SCORE(L)                                                                               \
  do {                                                                                                \
    if (p.score_type == 0) BH_LAUNCH((bh::detection_score_kernel<L, 0>), grid, block, 0, s, p, total); \
    else if (p.score_type == 1) BH_LAUNCH((bh::detection_score_kernel<L, 1>), grid, block, 0, s, p, total); \
    else BH_LAUNCH((bh::detection_score_kernel<L, 2>), grid, block, 0, s, p, total);                   \
  } while (0)
  if (wide) BH_DET_SCORE(16);
  else BH_DET_SCORE(4);
#undef BH_DET_SCORE
  int rc = bh_check_launch("detection_score_kernel");
  if (rc) return rc;
  const dim3 ngrid((unsigned)p.batch), nblock(bh::kDetNmsThreads);
  if (p.box_type == 0) BH_LAUNCH(bh::detection_nms_kernel<0>, ngrid, nblock, 0, s, p);
  else if (p.box_type == 1) BH_LAUNCH(bh::detection_nms_kernel<1>, ngrid, nblock, 0, s, p);
  else BH_LAUNCH(bh::detection_nms_kernel<2>, ngrid, nblock, 0, s, p);
  return bh_check_launch("detection_nms_kernel");
}
