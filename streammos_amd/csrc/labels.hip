// Per-frame label outputs of the overlapped sequence loop (streammos_amd/run_sequence.py) for gfx950.
//
// One launch reads a frame's labels once and
//   * writes the 32-bit words of the prediction file: the learning_map_inv value 0 / 9 / 251 of a 0/1/2 label
//     (val_StreamMOS.py:121-126), the label itself (the `_bf` file, val_StreamMOS_seg.py:141), or a copy of voted LUT words;
//   * counts the moving-IoU confusion against the frame's ground truth exactly as kitti.MovingIoU.add (utils/metric.py:18-58):
//     over the points whose mapped ground truth is not 0, tp / pred / gt of classes 1 and 2.
// Four points per lane per step (one 4-byte label load or one 16-byte word load, one 16-byte ground-truth load, one 16-byte
// word store); every predicate is a wave ballot, the counts stay in registers over the grid-stride loop and each wave adds
// them to the sequence's uint64 counters with one atomic per counter.  The counts are integers: the result equals numpy's.
#include "smos_common.h"

namespace smos {

enum LabelMode { kLutWords = 0, kRawWords = 1, kVotedWords = 2 };
constexpr int kLabelBlocksCap = 1024;

__device__ __forceinline__ int32_t lut_word(unsigned l) { return l == 1 ? 9 : (l == 2 ? 251 : 0); }
__device__ __forceinline__ int voted_class(int32_t w) { return w == 251 ? 2 : (w == 9 ? 1 : 0); }

__device__ __forceinline__ int mapped_gt(uint32_t word, const int32_t* __restrict__ gt_map, int32_t map_n) {
  const uint32_t sem = word & 0xFFFFu;
  return sem < (uint32_t)map_n ? gt_map[sem] : 0;   // the reader rejects ids outside the map; never read past it
}

// c[0..5] += tp1, tp2, pred1, pred2, gt1, gt2 of one point per lane.  Called by every lane of the wave (uniform control flow).
__device__ __forceinline__ void count_point(bool live, int p, int g, unsigned long long (&c)[6]) {
  const bool keep = live && g != 0;
  c[0] += __popcll(__ballot(keep && p == 1 && g == 1));
  c[1] += __popcll(__ballot(keep && p == 2 && g == 2));
  c[2] += __popcll(__ballot(keep && p == 1));
  c[3] += __popcll(__ballot(keep && p == 2));
  c[4] += __popcll(__ballot(keep && g == 1));
  c[5] += __popcll(__ballot(keep && g == 2));
}

template <int kMode>
__device__ __forceinline__ void load_one(const void* in, int64_t i, int& cls, int32_t& word) {
  if (kMode == kVotedWords) {
    word = static_cast<const int32_t*>(in)[i];
    cls = voted_class(word);
  } else {
    const unsigned l = static_cast<const uint8_t*>(in)[i];
    cls = (int)l;
    word = kMode == kLutWords ? lut_word(l) : (int32_t)l;
  }
}

template <int kMode>
__global__ __launch_bounds__(kBlock) void frame_labels(const void* __restrict__ in, int64_t n, int32_t* __restrict__ words,
                                                        const uint32_t* __restrict__ gt, const int32_t* __restrict__ gt_map,
                                                        int32_t map_n, unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  const int64_t wave = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);
  const bool counting = gt != nullptr;
  const int64_t n4 = n >> 2;
  unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
  // body: groups of 4 points; `base` is uniform over the wave, so every lane reaches every ballot
  for (int64_t base = wave * kWave; base < n4; base += waves * kWave) {
    const int64_t q = base + lane;
    const bool live = q < n4;
    int cls[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0};
    int32_t w[4] = {0, 0, 0, 0};
    if (live) {
      if (kMode == kVotedWords) {
        const int4 v = reinterpret_cast<const int4*>(in)[q];
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) cls[j] = voted_class(w[j]);
      } else {
        const uint32_t packed = reinterpret_cast<const uint32_t*>(in)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned l = (packed >> (8 * j)) & 0xFFu;
          cls[j] = (int)l;
          w[j] = kMode == kLutWords ? lut_word(l) : (int32_t)l;
        }
      }
      if (words) reinterpret_cast<int4*>(words)[q] = make_int4(w[0], w[1], w[2], w[3]);
      if (counting) {
        const uint4 t = reinterpret_cast<const uint4*>(gt)[q];
        g[0] = mapped_gt(t.x, gt_map, map_n), g[1] = mapped_gt(t.y, gt_map, map_n);
        g[2] = mapped_gt(t.z, gt_map, map_n), g[3] = mapped_gt(t.w, gt_map, map_n);
      }
    }
    if (counting) {
#pragma unroll
      for (int j = 0; j < 4; ++j) count_point(live, cls[j], g[j], c);
    }
  }
  // tail: the last n % 4 points, one per lane of the grid's first wave
  if (wave == 0 && (n & 3)) {
    const int64_t i = 4 * n4 + lane;
    const bool live = lane < (int)(n & 3);
    int cls = 0, g = 0;
    int32_t w = 0;
    if (live) {
      load_one<kMode>(in, i, cls, w);
      if (words) words[i] = w;
      if (counting) g = mapped_gt(gt[i], gt_map, map_n);
    }
    if (counting) count_point(live, cls, g, c);
  }
  if (counting && lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (c[k]) atomicAdd(counts + k, c[k]);
  }
}

static int launch_frame_labels(int mode, const void* in, int64_t n, int32_t* words, const uint32_t* gt, const int32_t* gt_map,
                               int32_t map_n, uint64_t* counts, hipStream_t stream, const char* what) {
  SMOS_REQUIRE(n >= 0, "%s: bad size %lld", what, (long long)n);
  SMOS_REQUIRE(!gt || (gt_map && map_n > 0 && counts), "%s: counting needs gt_map and counts", what);
  if (n == 0) return SMOS_OK;
  SMOS_REQUIRE(in, "%s: null labels", what);
  const uintptr_t in_align = mode == kVotedWords ? 15 : 3;
  SMOS_REQUIRE(((uintptr_t)in & in_align) == 0, "%s: labels must be %d-byte aligned", what, (int)in_align + 1);
  SMOS_REQUIRE(((uintptr_t)words & 15) == 0 && ((uintptr_t)gt & 15) == 0, "%s: words and gt must be 16-byte aligned", what);
  const int grid = grid_for((n >> 2) + 1, kBlock, kLabelBlocksCap);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (mode == kLutWords)
    hipLaunchKernelGGL(frame_labels<kLutWords>, dim3(grid), dim3(kBlock), 0, stream, in, n, words, gt, gt_map, map_n, cnt);
  else if (mode == kRawWords)
    hipLaunchKernelGGL(frame_labels<kRawWords>, dim3(grid), dim3(kBlock), 0, stream, in, n, words, gt, gt_map, map_n, cnt);
  else
    hipLaunchKernelGGL(frame_labels<kVotedWords>, dim3(grid), dim3(kBlock), 0, stream, in, n, words, gt, gt_map, map_n, cnt);
  return check_launch(what);
}

}  // namespace smos

using namespace smos;

extern "C" int smos_label_words(const uint8_t* labels, int64_t n, int32_t lut, int32_t* words, const uint32_t* gt,
                                const int32_t* gt_map, int32_t map_n, uint64_t* counts, smos_stream_t stream) {
  return launch_frame_labels(lut ? kLutWords : kRawWords, labels, n, words, gt, gt_map, map_n, counts, (hipStream_t)stream,
                             "label_words");
}

extern "C" int smos_label_count_voted(const int32_t* voted, int64_t n, int32_t* words, const uint32_t* gt, const int32_t* gt_map,
                                      int32_t map_n, uint64_t* counts, smos_stream_t stream) {
  return launch_frame_labels(kVotedWords, voted, n, words, gt, gt_map, map_n, counts, (hipStream_t)stream, "label_count_voted");
}
