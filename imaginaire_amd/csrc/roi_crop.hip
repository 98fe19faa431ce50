// k17: device-side part boxes and box crops (the pose recipes' face / hand discriminators).
//
// Replaces reference model_utils/fs_vid2vid.py:631-777 (get_face_bbox_for_output,
// get_hand_bbox_for_output, crop_face_from_output, crop_hand_from_output), which find each
// sample's box with .nonzero() + four .item() reads and then slice with Python integers: host
// state that a hipGraph cannot record and that would freeze the capture-time box into every
// replay. Here the box never leaves the device:
//   * part_bbox: min / max of y and x over the pixels a predicate selects, per (sample, part),
//     in two stages: workgroups reduce 4096-element chunks of the plane (16-byte loads where
//     it is contiguous, per-lane min / max, wave shuffle, LDS across waves) to one extent
//     each, then one wave per (sample, part) merges the chunks and one lane applies the
//     reference's box rule in integer arithmetic and stores five ints. (One workgroup per
//     plane took 42 us at 3 x 512 x 512.) No atomics and no zeroed buffer: the captured graph
//     gets kernel nodes only;
//   * roi_crop_fwd: crop to the box read from device memory + bilinear resize
//     (align_corners=True, PyTorch's source-index rule) of the last 3 channels, all samples in
//     one launch, fp32 accumulation;
//   * roi_crop_bwd: a GATHER over the whole dimage: every input pixel sums the output
//     pixels whose taps touch it (taps recomputed with the forward's expressions) and pixels
//     outside the box or in earlier channels store 0, so the caller zeroes nothing and the
//     result is deterministic.
#include "common.h"

#include <climits>
#include <type_traits>

namespace iamd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 4;
constexpr int kChunkElems = 4096;  // label elements per stage-1 workgroup (16 per thread)
constexpr int kMaxChunks = 256;

struct Parts {
  int ch[kMaxParts];
};

// box rules (reference fs_vid2vid.py:661-714 face, :743-777 hand)
constexpr int kFaceOpenPose = 0;
constexpr int kFaceDensePose = 1;
constexpr int kHand = 2;

struct MinMax {
  int y0, y1, x0, x1;
};

// branch-free: a pixel that misses the predicate merges the identity of min / max
__device__ __forceinline__ void mm_add(MinMax& m, bool hit, int y, int x) {
  m.y0 = min(m.y0, hit ? y : INT_MAX);
  m.y1 = max(m.y1, hit ? y : -1);
  m.x0 = min(m.x0, hit ? x : INT_MAX);
  m.x1 = max(m.x1, hit ? x : -1);
}

// centre clamped as the Python does: max(len // 2, min(dim - 1 - len // 2, c))
__device__ __forceinline__ int clamp_centre(int c, int len, int dim) {
  return max(len / 2, min(dim - 1 - len / 2, c));
}

// ys, ye, xs, xe, valid from the selected pixels' extent (empty: y1 < 0). Every operand is a
// non-negative int, so C division is Python's floor division.
__device__ __forceinline__ void box_rule(const MinMax& m, int rule, int h, int w,
                                         int crop_smaller, int* __restrict__ out) {
  const bool empty = m.y1 < 0;
  int yc, xc, len, valid = 1;
  if (rule == kHand) {
    len = h / 64 * 8;
    valid = empty ? 0 : 1;
    yc = clamp_centre(empty ? 0 : (m.y0 + m.y1) / 2, len, h);
    xc = clamp_centre(empty ? 0 : (m.x0 + m.x1) / 2, len, w);
  } else if (empty) {
    len = h / 32 * 8;
    yc = h / 4;
    xc = w / 2;
  } else {
    xc = (m.x0 + m.x1) / 2;
    if (rule == kFaceOpenPose) {
      yc = (3 * m.y0 + 2 * m.y1) / 5;
      len = (5 * (m.x1 - m.x0)) / 2;  // int((xe - xs) * 2.5)
    } else {
      yc = (m.y0 + m.y1) / 2;
      len = (5 * (m.y1 - m.y0)) / 4;  // int((ye - ys) * 1.25)
    }
    len = min(w, max(32, len));
    yc = clamp_centre(yc, len, h);
    xc = clamp_centre(xc, len, w);
  }
  out[0] = yc - len / 2 + crop_smaller;
  out[1] = yc + len / 2 - crop_smaller;
  out[2] = xc - len / 2 + crop_smaller;
  out[3] = xc + len / 2 - crop_smaller;
  out[4] = valid;
}

__device__ __forceinline__ void mm_merge(MinMax& m, int y0, int y1, int x0, int x1) {
  m.y0 = min(m.y0, y0);
  m.y1 = max(m.y1, y1);
  m.x0 = min(m.x0, x0);
  m.x1 = max(m.x1, x1);
}

__device__ __forceinline__ void mm_wave_reduce(MinMax& m) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1)
    mm_merge(m, __shfl_down(m.y0, o, kWave), __shfl_down(m.y1, o, kWave),
             __shfl_down(m.x0, o, kWave), __shfl_down(m.x1, o, kWave));
}

// stage 1: workgroup (chunk, part, b) reduces its share of one label plane to
// partial[b, part, chunk] = (y0, y1, x0, x1). Every slot is written: nothing to zero.
template <typename T>
__global__ void __launch_bounds__(kThreads)
part_minmax_kernel(const T* __restrict__ label, int* __restrict__ partial, Parts parts, int H,
                   int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int eq, float ref) {
  constexpr int V = VecN<T>::N;
  const int chunk = blockIdx.x, nchunks = gridDim.x, part = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int ch = part == 0 ? parts.ch[0] : part == 1 ? parts.ch[1] : part == 2 ? parts.ch[2]
                                                                                : parts.ch[3];
  const T* __restrict__ p = label + b * sb + ch * sc;
  MinMax m{INT_MAX, -1, INT_MAX, -1};
  auto hit = [&](T v) {
    const float f = to_f<T>(v);
    return eq ? f == ref : f > ref;
  };
  const int n = H * W;
  if (sw == 1 && sh == W) {
    // the plane is one flat run of H * W elements: scalar head up to the first 16-byte
    // boundary, 16-byte body shared out among the chunks, scalar tail
    const int mis = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) % V);
    const int head = min(n, (V - mis) % V);
    const int nvec = (n - head) / V;
    const int tail = head + nvec * V;
    if (chunk == 0) {
      if (tid < head) mm_add(m, hit(p[tid]), tid / W, tid % W);
      if (tail + tid < n) mm_add(m, hit(p[tail + tid]), (tail + tid) / W, (tail + tid) % W);
    }
    const int per = (nvec + nchunks - 1) / nchunks;
    const int k1 = min(nvec, (chunk + 1) * per);
#pragma unroll 2
    for (int k = chunk * per + tid; k < k1; k += kThreads) {
      const int i = head + k * V;
      const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(p + i);
      int y = i / W, x = i - y * W;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        mm_add(m, hit(pk.v[j]), y, x);
        const bool wrap = ++x == W;
        x = wrap ? 0 : x;
        y += wrap ? 1 : 0;
      }
    }
  } else {
    const int per = (n + nchunks - 1) / nchunks;
    const int i1 = min(n, (chunk + 1) * per);
#pragma unroll 2
    for (int i = chunk * per + tid; i < i1; i += kThreads) {
      const int y = i / W, x = i - y * W;
      mm_add(m, hit(p[y * sh + x * sw]), y, x);
    }
  }
  mm_wave_reduce(m);
  __shared__ int sh_mm[kThreads / kWave][4];
  if ((tid & (kWave - 1)) == 0) {
    int* s = sh_mm[tid / kWave];
    s[0] = m.y0;
    s[1] = m.y1;
    s[2] = m.x0;
    s[3] = m.x1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kThreads / kWave; ++k)
      mm_merge(m, sh_mm[k][0], sh_mm[k][1], sh_mm[k][2], sh_mm[k][3]);
    int* __restrict__ out = partial + (((int64_t)b * gridDim.y + part) * nchunks + chunk) * 4;
    out[0] = m.y0;
    out[1] = m.y1;
    out[2] = m.x0;
    out[3] = m.x1;
  }
}

// stage 2: one wave per (sample, part) merges the chunks' extents and applies the box rule
__global__ void __launch_bounds__(kWave)
part_box_kernel(const int* __restrict__ partial, int* __restrict__ boxes, int nchunks, int rule,
                int H, int W, int crop_smaller) {
  const int* __restrict__ src = partial + (int64_t)blockIdx.x * nchunks * 4;
  MinMax m{INT_MAX, -1, INT_MAX, -1};
  for (int k = threadIdx.x; k < nchunks; k += kWave)
    mm_merge(m, src[k * 4], src[k * 4 + 1], src[k * 4 + 2], src[k * 4 + 3]);
  mm_wave_reduce(m);
  if (threadIdx.x == 0) box_rule(m, rule, H, W, crop_smaller, boxes + (int64_t)blockIdx.x * 5);
}

// ---- crop + resize ------------------------------------------------------------------------
// One axis of one box: the box clipped to the image as Python slicing clips it, and PyTorch's
// align_corners=True source scale of the clipped extent (area_pixel_compute_scale in fp32).
struct Span {
  int start, in;  // first source index, clipped extent (<= 0: nothing to read)
  float scale;
};

__device__ __forceinline__ Span make_span(int s, int e, int dim, int out) {
  Span a;
  a.start = max(s, 0);
  a.in = min(e, dim) - a.start;
  a.scale = out > 1 ? (float)(a.in - 1) / (float)(out - 1) : 0.f;
  return a;
}

// taps of output index o: (i0, i1, lambda), relative to the span's start
__device__ __forceinline__ void taps(const Span& a, int o, int& i0, int& i1, float& l) {
  const float src = a.scale * (float)o;
  i0 = (int)src;
  i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
  l = src - (float)i0;
}

// out[bn, c, oy, ox .. ox + V): grid.y = bn, so the box is uniform over the workgroup
template <typename T, int V>
__global__ void __launch_bounds__(kThreads)
roi_crop_fwd_kernel(const T* __restrict__ img, const int* __restrict__ boxes,
                    T* __restrict__ out, int n_parts, int C, int H, int W, int64_t sb,
                    int64_t sc, int64_t sh, int64_t sw, int oh, int ow) {
  const int bn = blockIdx.y;
  const int* __restrict__ box = boxes + (int64_t)bn * 5;
  const Span ay = make_span(box[0], box[1], H, oh);
  const Span ax = make_span(box[2], box[3], W, ow);
  const bool none = ay.in <= 0 || ax.in <= 0;
  const T* __restrict__ base = img + (bn / n_parts) * sb + (C - 3) * sc;
  const int owv = ow / V;
  const int n = 3 * oh * owv;
  for (int t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
    const int xv = t % owv;
    const int oy = (t / owv) % oh;
    const int c = t / (owv * oh);
    float o[V];
    if (none) {
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = 0.f;
    } else {
      int y0, y1;
      float ly;
      taps(ay, oy, y0, y1, ly);
      const T* __restrict__ r0 = base + c * sc + (ay.start + y0) * sh;
      const T* __restrict__ r1 = base + c * sc + (ay.start + y1) * sh;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        int x0, x1;
        float lx;
        taps(ax, xv * V + j, x0, x1, lx);
        const int64_t o0 = (ax.start + x0) * sw, o1 = (ax.start + x1) * sw;
        // PyTorch's upsample_bilinear2d expression
        o[j] = (1.f - ly) * ((1.f - lx) * to_f<T>(r0[o0]) + lx * to_f<T>(r0[o1])) +
               ly * ((1.f - lx) * to_f<T>(r1[o0]) + lx * to_f<T>(r1[o1]));
      }
    }
    store_vec<T, V>(out + (((int64_t)bn * 3 + c) * oh + oy) * ow + xv * V, o);
  }
}

// [lo, hi]: a window of outputs of one axis that holds every output reading a source index
// in [i_lo, i_hi] (relative to the span). Output o reads i only if scale * o lies in
// (i - 1, i + 1): the window is one wider than the preimage of that interval, and the forward's
// own taps decide inside it.
__device__ __forceinline__ void reader_window(const Span& a, int out, int i_lo, int i_hi,
                                              int& lo, int& hi) {
  lo = 0;
  hi = out - 1;
  if (a.scale > 0.f) {
    const float inv = 1.f / a.scale;
    lo = max(0, (int)floorf(((float)i_lo - 1.f) * inv) - 1);
    hi = min(out - 1, (int)ceilf(((float)i_hi + 1.f) * inv) + 1);
  }
}

// weight with which an output whose taps are (i0, i1, l) reads source index i
__device__ __forceinline__ float tap_weight(int i0, int i1, float l, int i) {
  return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

// dimg[b, c, iy, ix .. ix + V) for every pixel of the image
template <typename T, int V>
__global__ void __launch_bounds__(kThreads)
roi_crop_bwd_kernel(const T* __restrict__ dy, const int* __restrict__ boxes,
                    T* __restrict__ dimg, int n_parts, int B, int C, int H, int W, int64_t sb,
                    int64_t sc, int64_t sh, int64_t sw, int oh, int ow) {
  const int wv = W / V;
  const int64_t n = (int64_t)B * C * H * wv;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * kThreads) {
    const int xv = (int)(t % wv);
    int64_t q = t / wv;
    const int iy = (int)(q % H);
    q /= H;
    const int c = (int)(q % C);
    const int b = (int)(q / C);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (c >= C - 3) {
      for (int part = 0; part < n_parts; ++part) {
        const int bn = b * n_parts + part;
        const int* __restrict__ box = boxes + (int64_t)bn * 5;
        const Span ay = make_span(box[0], box[1], H, oh);
        const Span ax = make_span(box[2], box[3], W, ow);
        const int ry = iy - ay.start;
        if (ay.in <= 0 || ax.in <= 0 || ry < 0 || ry >= ay.in) continue;
        const T* __restrict__ g = dy + ((int64_t)bn * 3 + (c - (C - 3))) * oh * ow;
        // the thread's V pixels share one window of output columns; each output's taps are
        // computed once and matched against every pixel
        const int rx0 = xv * V - ax.start;
        if (rx0 + V <= 0 || rx0 >= ax.in) continue;
        int ylo, yhi, xlo, xhi;
        reader_window(ay, oh, ry, ry, ylo, yhi);
        reader_window(ax, ow, max(rx0, 0), min(rx0 + V - 1, ax.in - 1), xlo, xhi);
        for (int oy = ylo; oy <= yhi; ++oy) {
          int y0, y1;
          float ly;
          taps(ay, oy, y0, y1, ly);
          const float wy = tap_weight(y0, y1, ly, ry);
          if (wy == 0.f) continue;
          const T* __restrict__ row = g + (int64_t)oy * ow;
          for (int ox = xlo; ox <= xhi; ++ox) {
            int x0, x1;
            float lx;
            taps(ax, ox, x0, x1, lx);
            const float gv = to_f<T>(row[ox]);
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float wx = tap_weight(x0, x1, lx, rx0 + j);
              if (wx != 0.f) acc[j] = fmaf(wy * wx, gv, acc[j]);
            }
          }
        }
      }
    }
    T* __restrict__ dst = dimg + b * sb + c * sc + iy * sh + (int64_t)xv * V * sw;
    if (V > 1) {
      store_vec<T, V>(dst, acc);
    } else {
      dst[0] = from_f<T>(acc[0]);
    }
  }
}

void check_image(const at::Tensor& t, const char* what) {
  IAMD_CHECK(t.is_cuda() && t.dim() == 4, what, ": 4-D CUDA tensor expected");
  IAMD_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat, what,
             ": bf16 or fp32 expected");
  IAMD_CHECK(t.numel() < INT_MAX, what, ": tensor too large");
}

void check_boxes(const at::Tensor& boxes, int64_t B, const char* what) {
  IAMD_CHECK(boxes.is_cuda() && boxes.scalar_type() == at::kInt && boxes.dim() == 3 &&
                 boxes.size(0) == B && boxes.size(1) >= 1 && boxes.size(2) == 5 &&
                 boxes.is_contiguous(),
             what, ": boxes must be a contiguous int32 [B, n, 5] CUDA tensor");
}

// rows of V elements can be accessed with one 16-byte instruction: unit stride along W, every
// other stride and the base a multiple of V elements
template <typename T>
bool rows_vectorizable(const at::Tensor& t) {
  constexpr int V = VecN<T>::N;
  return t.stride(3) == 1 && t.size(3) % V == 0 && t.stride(0) % V == 0 &&
         t.stride(1) % V == 0 && t.stride(2) % V == 0 &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// f(tag) with a null pointer of the tensor's element type (fp32 or bf16: check_image)
template <typename F>
void dispatch(at::ScalarType t, F f) {
  if (t == at::kFloat)
    f(static_cast<float*>(nullptr));
  else
    f(static_cast<__hip_bfloat16*>(nullptr));
}

int grid_for(int64_t n) { return (int)std::min<int64_t>((n + kThreads - 1) / kThreads, 2048); }

}  // namespace

// int32 [B, n_parts, 5] = (ys, ye, xs, xe, valid) per (sample, part channel): the box rule
// `rule` applied to the extent of the pixels with label > ref (eq = false) or == ref.
at::Tensor part_bbox(const at::Tensor& label, std::vector<int64_t> channels, int64_t rule,
                     bool eq, double ref, int64_t crop_smaller) {
  check_image(label, "part_bbox");
  const int B = (int)label.size(0), C = (int)label.size(1);
  const int H = (int)label.size(2), W = (int)label.size(3);
  IAMD_CHECK(!channels.empty() && (int)channels.size() <= kMaxParts,
             "part_bbox: 1 to ", kMaxParts, " part channels expected");
  IAMD_CHECK(rule >= kFaceOpenPose && rule <= kHand, "part_bbox: unknown rule ", rule);
  Parts parts;
  for (size_t k = 0; k < channels.size(); ++k) {
    IAMD_CHECK(channels[k] >= 0 && channels[k] < C, "part_bbox: channel out of range");
    parts.ch[k] = (int)channels[k];
  }
  const int n = (int)channels.size();
  auto boxes = at::empty({B, n, 5}, label.options().dtype(at::kInt));
  if (B == 0) return boxes;
  IAMD_CHECK(H > 0 && W > 0, "part_bbox: empty label plane");
  IAMD_CHECK(B <= 65535, "part_bbox: batch too large");
  const int nchunks = (int)std::min<int64_t>(
      ((int64_t)H * W + kChunkElems - 1) / kChunkElems, kMaxChunks);
  auto partial = at::empty({B, n, nchunks, 4}, boxes.options());
  dispatch(label.scalar_type(), [&](auto tag) {
    using scalar_t = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((part_minmax_kernel<scalar_t>), dim3(nchunks, n, B), dim3(kThreads), 0,
                       stream(), reinterpret_cast<const scalar_t*>(label.data_ptr()),
                       partial.data_ptr<int>(), parts, H, W, label.stride(0), label.stride(1),
                       label.stride(2), label.stride(3), (int)eq, (float)ref);
  });
  IAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(part_box_kernel, dim3(B * n), dim3(kWave), 0, stream(),
                     partial.data_ptr<int>(), boxes.data_ptr<int>(), nchunks, (int)rule, H, W,
                     (int)crop_smaller);
  IAMD_LAUNCH_CHECK();
  return boxes;
}

// out[B * n, 3, oh, ow] (contiguous): the last 3 channels of image[b] cropped to boxes[b, k]
// (read on the device) and resized bilinearly, align_corners=True
at::Tensor roi_crop_fwd(const at::Tensor& image, const at::Tensor& boxes, int64_t oh,
                        int64_t ow) {
  check_image(image, "roi_crop_fwd");
  const int B = (int)image.size(0), C = (int)image.size(1);
  const int H = (int)image.size(2), W = (int)image.size(3);
  IAMD_CHECK(C >= 3, "roi_crop_fwd: at least 3 channels expected");
  IAMD_CHECK(oh > 0 && ow > 0, "roi_crop_fwd: empty output size");
  check_boxes(boxes, B, "roi_crop_fwd");
  const int n = (int)boxes.size(1);
  IAMD_CHECK((int64_t)B * n <= 65535, "roi_crop_fwd: more than 65535 boxes");
  auto out = at::empty({(int64_t)B * n, 3, oh, ow}, image.options());
  if (B == 0) return out;
  dispatch(image.scalar_type(), [&](auto tag) {
    using scalar_t = std::remove_pointer_t<decltype(tag)>;
    constexpr int V = VecN<scalar_t>::N;
    auto launch = [&](auto vec) {
      constexpr int kV = decltype(vec)::value;
      hipLaunchKernelGGL((roi_crop_fwd_kernel<scalar_t, kV>),
                         dim3(grid_for(3 * oh * (ow / kV)), B * n), dim3(kThreads), 0, stream(),
                         reinterpret_cast<const scalar_t*>(image.data_ptr()),
                         boxes.data_ptr<int>(), reinterpret_cast<scalar_t*>(out.data_ptr()), n,
                         C, H, W, image.stride(0), image.stride(1), image.stride(2),
                         image.stride(3), (int)oh, (int)ow);
    };
    if (ow % V == 0)
      launch(std::integral_constant<int, V>());
    else
      launch(std::integral_constant<int, 1>());
  });
  IAMD_LAUNCH_CHECK();
  return out;
}

// dimage (the strides of `like`, which must be dense) from dy[B * n, 3, oh, ow]: every element
// is written (0 outside the boxes and in the channels before the last 3)
at::Tensor roi_crop_bwd(const at::Tensor& dy, const at::Tensor& boxes, const at::Tensor& like) {
  check_image(dy, "roi_crop_bwd");
  IAMD_CHECK(like.dim() == 4 && like.is_non_overlapping_and_dense(),
             "roi_crop_bwd: dense 4-D image expected");
  const int B = (int)like.size(0), C = (int)like.size(1);
  const int H = (int)like.size(2), W = (int)like.size(3);
  check_boxes(boxes, B, "roi_crop_bwd");
  const int n = (int)boxes.size(1);
  IAMD_CHECK(dy.is_contiguous() && dy.size(0) == (int64_t)B * n && dy.size(1) == 3 && C >= 3 &&
                 dy.scalar_type() == like.scalar_type(),
             "roi_crop_bwd: dy must be a contiguous [B * n, 3, oh, ow] tensor of the image dtype");
  auto dimg = at::empty_strided(like.sizes(), like.strides(), dy.options());
  check_image(dimg, "roi_crop_bwd");
  if (dimg.numel() == 0) return dimg;
  const int oh = (int)dy.size(2), ow = (int)dy.size(3);
  dispatch(dy.scalar_type(), [&](auto tag) {
    using scalar_t = std::remove_pointer_t<decltype(tag)>;
    constexpr int V = VecN<scalar_t>::N;
    auto launch = [&](auto vec) {
      constexpr int kV = decltype(vec)::value;
      hipLaunchKernelGGL((roi_crop_bwd_kernel<scalar_t, kV>),
                         dim3(grid_for(dimg.numel() / kV)), dim3(kThreads), 0, stream(),
                         reinterpret_cast<const scalar_t*>(dy.data_ptr()), boxes.data_ptr<int>(),
                         reinterpret_cast<scalar_t*>(dimg.data_ptr()), n, B, C, H, W,
                         dimg.stride(0), dimg.stride(1), dimg.stride(2), dimg.stride(3), oh, ow);
    };
    if (rows_vectorizable<scalar_t>(dimg))
      launch(std::integral_constant<int, V>());
    else
      launch(std::integral_constant<int, 1>());
  });
  IAMD_LAUNCH_CHECK();
  return dimg;
}

}  // namespace iamd
