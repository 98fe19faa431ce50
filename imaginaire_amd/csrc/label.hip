// k19: packed label maps -> the dense label tensor the networks read, in one launch.
//
// A dataset with ``packed_labels`` ships every one-hot label type as ONE index plane (uint8, or
// int16 above 255 classes; value n = "don't care / out of range") and keeps only the dense types
// (edge maps, instance maps, ...) as fp32 channels. This kernel writes the whole
// [B, C (+ zero pad), Ho, Wo] tensor from them: per layout segment a one-hot channel c is 1 where
// idx == c (idx == n lights the don't-care channel when the segment has one and nothing
// otherwise), dense channels are copied, channels [C, Cp) are zeros. With a target size every
// output pixel reads the source pixel nearest_src names (resize_index.h, the rule of the k12
// nearest resize), so the result equals interpolate(expanded) bit for bit: a nearest resize only
// moves values.
//
// The kernel is a pure store stream (0.4 GB per batch of 4 at 185 x 256 x 512 fp32 against 0.5 MB
// of indices read). The output, NCHW or packed NHWC, is one dense array, and it is written as
// such: lane q owns elements [q * VEC, (q + 1) * VEC) of the flat array, VEC = 4 fp32 / 8 bf16,
// one aligned 16-byte store whatever C and Wo are (185 channels, odd widths). In NHWC a piece is
// VEC consecutive channels of a pixel, in NCHW VEC consecutive pixels of a channel row; where C
// or Wo is no multiple of VEC a piece runs on into the next pixel / row, which the per-element
// cursor below follows, and the only scalar stores are the < VEC elements at the very end of
// the tensor. The cursor keeps the segment of the current channel and the index value of the
// current source pixel in registers and reloads either only when it is left. Plain stores: every
// 128-byte line is written whole by consecutive lanes and is read next by a conv.
// No atomics, no LDS, no scratch; the layout table travels by value in the launch arguments and
// nothing is read on the host, so the launch can be captured into a hipGraph.
#include "common.h"
#include "resize_index.h"

namespace iamd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxLabelSegs = 16;

// Segment s covers output channels [c0[s], c0[s] + cn[s]). kind 0: one-hot of index plane
// src[s]; kind 1: dense channels [src[s], src[s] + cn[s]).
struct LabelTab {
  int nseg;
  int c0[kMaxLabelSegs];
  int cn[kMaxLabelSegs];
  int src[kMaxLabelSegs];
  int kind[kMaxLabelSegs];
};

struct LabelGeom {
  int B, K, Cd, C, Cp;  // index planes, dense channels, valid / padded output channels
  Axis ay, ax;          // source -> output, nearest
};

// Elements [e0, e0 + NV) of the flat output (all of them inside the tensor).
template <typename T, typename I, int NV, bool NHWC>
__device__ __forceinline__ void label_piece(const I* __restrict__ idx,
                                            const float* __restrict__ dense, const LabelTab& t,
                                            const LabelGeom& g, int64_t e0, T (&out)[NV]) {
  const int Ho = g.ay.out, Wo = g.ax.out;
  const int64_t HW = (int64_t)g.ay.in * g.ax.in;
  // coordinates of element e0
  int b, c, oy, ox;
  {
    int64_t r = e0;
    if (NHWC) {
      c = (int)(r % g.Cp); r /= g.Cp;
      ox = (int)(r % Wo); r /= Wo;
      oy = (int)(r % Ho);
      b = (int)(r / Ho);
    } else {
      ox = (int)(r % Wo); r /= Wo;
      oy = (int)(r % Ho); r /= Ho;
      c = (int)(r % g.Cp);
      b = (int)(r / g.Cp);
    }
  }
  // cursor: segment [lo, hi) of kind kd reading src; v = index value at the source pixel
  int lo = 0, hi = 0, kd = 2, src = 0, v = -1;
  int64_t sp = 0;  // offset of the source pixel in plane 0 of its sample
  bool new_pixel = true;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (new_pixel) sp = (int64_t)nearest_src(g.ay, oy) * g.ax.in + nearest_src(g.ax, ox);
    const bool new_seg = c < lo || c >= hi;
    if (new_seg) {
      lo = g.C; hi = g.Cp; kd = 2;  // the zero tail unless a segment claims c
      for (int s = 0; s < t.nseg; ++s) {
        if (c >= t.c0[s] && c < t.c0[s] + t.cn[s]) {
          lo = t.c0[s]; hi = lo + t.cn[s]; kd = t.kind[s]; src = t.src[s];
        }
      }
    }
    float val = 0.f;
    if (kd == 0) {
      if (new_pixel || new_seg) v = (int)idx[((int64_t)b * g.K + src) * HW + sp];
      val = v == c - lo ? 1.f : 0.f;
    } else if (kd == 1) {
      val = dense[((int64_t)b * g.Cd + src + (c - lo)) * HW + sp];
    }
    out[j] = from_f<T>(val);
    // next element of the flat output
    if (NHWC) {
      new_pixel = false;
      if (++c == g.Cp) {
        c = 0; new_pixel = true;
        if (++ox == Wo) { ox = 0; if (++oy == Ho) { oy = 0; ++b; } }
      }
    } else {
      new_pixel = true;
      if (++ox == Wo) {
        ox = 0;
        if (++oy == Ho) { oy = 0; if (++c == g.Cp) { c = 0; ++b; } }
      }
    }
  }
}

template <typename T, typename I, int VEC, bool NHWC>
__global__ void __launch_bounds__(kThreads)
label_expand(const I* __restrict__ idx, const float* __restrict__ dense, T* __restrict__ y,
             LabelTab t, LabelGeom g) {
  const int64_t n = (int64_t)g.B * g.Cp * g.ay.out * g.ax.out;
  const int64_t pieces = n / VEC;
  for (int64_t q = blockIdx.x * (int64_t)kThreads + threadIdx.x; q < pieces;
       q += (int64_t)gridDim.x * kThreads) {
    Pack<T, VEC> out;
    label_piece<T, I, VEC, NHWC>(idx, dense, t, g, q * VEC, out.v);
    *reinterpret_cast<Pack<T, VEC>*>(y + q * VEC) = out;
  }
  // the n % VEC elements after the last whole piece: one scalar store each
  const int64_t e = pieces * VEC + threadIdx.x;
  if (blockIdx.x == 0 && e < n) {
    T one[1];
    label_piece<T, I, 1, NHWC>(idx, dense, t, g, e, one);
    y[e] = one[0];
  }
}

template <typename T, typename I>
void launch(const void* idx, const float* dense, at::Tensor& y, const LabelTab& t,
            const LabelGeom& g, bool nhwc) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t pieces = y.numel() / VEC;  // block 0 also writes the < VEC tail elements
  const int grid = (int)std::min<int64_t>(pieces / kThreads + 1, 1 << 20);
  T* yp = reinterpret_cast<T*>(y.data_ptr());
  const I* ip = reinterpret_cast<const I*>(idx);
  if (nhwc)
    hipLaunchKernelGGL((label_expand<T, I, VEC, true>), dim3(grid), dim3(kThreads), 0, stream(),
                       ip, dense, yp, t, g);
  else
    hipLaunchKernelGGL((label_expand<T, I, VEC, false>), dim3(grid), dim3(kThreads), 0, stream(),
                       ip, dense, yp, t, g);
  IAMD_LAUNCH_CHECK();
}

}  // namespace

// y[B, pad_to, Ho, Wo] (bf16 / fp32; NCHW or packed channels-last) from idx[B, K, H, W] (uint8 /
// int16, contiguous; undefined when the layout has no one-hot segment) and dense[B, Cd, H, W]
// (fp32, contiguous; undefined when it has no dense one). Segment i: kind[i] (0 one-hot, 1 dense),
// cn[i] output channels, src[i] = index plane or first dense channel; segments tile [0, C) in
// order. scale_* = PyTorch's nearest source scale (in / out).
at::Tensor label_expand(const c10::optional<at::Tensor>& idx,
                        const c10::optional<at::Tensor>& dense, std::vector<int64_t> kind,
                        std::vector<int64_t> cn, std::vector<int64_t> src, int64_t pad_to,
                        int64_t Ho, int64_t Wo, double scale_h, double scale_w,
                        at::ScalarType dtype, bool channels_last) {
  const bool has_i = idx.has_value() && idx->defined();
  const bool has_d = dense.has_value() && dense->defined();
  IAMD_CHECK(has_i || has_d, "label_expand: no input");
  const at::Tensor& ref = has_i ? *idx : *dense;
  IAMD_CHECK(ref.is_cuda() && ref.dim() == 4, "label_expand: 4-D GPU tensors expected");
  if (has_i)
    IAMD_CHECK(idx->is_contiguous() &&
                   (idx->scalar_type() == at::kByte || idx->scalar_type() == at::kShort),
               "label_expand: contiguous uint8 / int16 index planes expected");
  if (has_d)
    IAMD_CHECK(dense->is_cuda() && dense->dim() == 4 && dense->is_contiguous() &&
                   dense->scalar_type() == at::kFloat && dense->device() == ref.device() &&
                   dense->size(0) == ref.size(0) && dense->size(2) == ref.size(2) &&
                   dense->size(3) == ref.size(3),
               "label_expand: dense must be contiguous fp32 [B, Cd, H, W] matching idx");
  IAMD_CHECK(dtype == at::kFloat || dtype == at::kBFloat16, "label_expand: fp32 or bf16 output");
  const size_t ns = kind.size();
  IAMD_CHECK(ns >= 1 && ns <= (size_t)kMaxLabelSegs && cn.size() == ns && src.size() == ns,
             "label_expand: 1 .. ", kMaxLabelSegs, " segments expected");
  LabelGeom g;
  g.B = (int)ref.size(0);
  g.K = has_i ? (int)idx->size(1) : 0;
  g.Cd = has_d ? (int)dense->size(1) : 0;
  LabelTab t;
  t.nseg = (int)ns;
  int64_t c = 0;
  for (int s = 0; s < kMaxLabelSegs; ++s) t.c0[s] = t.cn[s] = t.src[s] = t.kind[s] = 0;
  for (size_t s = 0; s < ns; ++s) {
    IAMD_CHECK(cn[s] >= 1 && (kind[s] == 0 || kind[s] == 1), "label_expand: bad segment ", s);
    // every read the kernel makes through the table stays inside idx / dense
    IAMD_CHECK(src[s] >= 0 && (kind[s] == 0 ? src[s] < g.K : src[s] + cn[s] <= g.Cd),
               "label_expand: segment ", s, " reads outside its input");
    t.c0[s] = (int)c; t.cn[s] = (int)cn[s]; t.src[s] = (int)src[s]; t.kind[s] = (int)kind[s];
    c += cn[s];
  }
  IAMD_CHECK(pad_to >= c && Ho >= 1 && Wo >= 1, "label_expand: pad_to below the channel count");
  g.C = (int)c;
  g.Cp = (int)pad_to;
  g.ay = make_axis(ref.size(2), Ho, scale_h, false);
  g.ax = make_axis(ref.size(3), Wo, scale_w, false);
  IAMD_CHECK((int64_t)g.B * g.Cp * Ho * Wo < ((int64_t)1 << 40) && ref.size(2) >= 1 &&
                 ref.size(3) >= 1 && scale_h >= 0.0 && scale_w >= 0.0,
             "label_expand: bad geometry");
  auto opt = ref.options().dtype(dtype);
  auto y = channels_last
               ? at::empty({g.B, g.Cp, Ho, Wo}, opt.memory_format(at::MemoryFormat::ChannelsLast))
               : at::empty({g.B, g.Cp, Ho, Wo}, opt);
  if (y.numel() == 0) return y;
  const void* ip = has_i ? idx->data_ptr() : nullptr;
  const float* dp = has_d ? dense->data_ptr<float>() : nullptr;
  const bool wide = has_i && idx->scalar_type() == at::kShort;
  if (dtype == at::kBFloat16) {
    if (wide) launch<__hip_bfloat16, int16_t>(ip, dp, y, t, g, channels_last);
    else launch<__hip_bfloat16, uint8_t>(ip, dp, y, t, g, channels_last);
  } else {
    if (wide) launch<float, int16_t>(ip, dp, y, t, g, channels_last);
    else launch<float, uint8_t>(ip, dp, y, t, g, channels_last);
  }
  return y;
}

}  // namespace iamd
