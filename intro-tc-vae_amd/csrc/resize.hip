// PIL-exact bicubic resize of uint8 image tables on the device (dataset.py:78-79,144-145 and load_image's last line:
// Image.resize(..., Image.BICUBIC) per sample on the host).  Pillow's 8-bit resampler is integer arithmetic once its
// coefficient tables exist: per axis, out = clamp((2^21 + sum_t src[min + t] * k[t]) >> 22, 0, 255) with int32 k in 2^-22
// units, the horizontal pass first (to uint8), the vertical pass on its result.  The tables ("plans") are made on the
// host in fp64 exactly as Pillow makes them (hipvae/resize.py); nothing here is floating point before the final / 255.
//
// One block per (image, plane, band of output rows).  The block copies the source rows its band needs into LDS, runs
// the horizontal pass from there into a second uint8 LDS array [rows x Wout] and the vertical pass from that array to
// global memory.  Neighbouring bands recompute the horizontal rows they share (ky - scale rows of a band's
// band * scale + ky).  Coefficients are staged in LDS once per block: in the vertical pass the lanes that share an
// output row read one address (a broadcast), in the horizontal pass lane x reads row x of a table whose row length kx is
// odd, so 32 neighbouring lanes hit 32 banks.
#include "common.h"

namespace itcv {

struct ResizeArgs {
  const unsigned char* table;
  long long num_images;
  int planes, Hin, Win;
  const long long* idx;
  const unsigned char* flip;
  const int* xbounds;
  const int* xcoef;
  int kx;
  const int* ybounds;
  const int* ycoef;
  int ky;
  int Hout, Wout;
  void* out;
  int* flags;
  int band, bands;        // output rows per block, blocks per plane
  int maxrows;            // source rows the LDS arrays hold
  int SW, MW;             // LDS row strides of the source rows and of the horizontal result (multiples of 4)
  int lw_in, lw_out, lw_quad;   // log2 of the lanes that walk one row: staging, horizontal pass, vertical pass
  int vec_in, vec_out;    // 16-byte loads of the source / 16-byte (fp32) or 4-byte (uint8) stores of the result
};

__device__ __forceinline__ int to_byte(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <bool F32>
__global__ __launch_bounds__(256) void resize_u8_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const unsigned int blk = blockIdx.x;
  const unsigned int band_i = blk % (unsigned int)a.bands, q = blk / (unsigned int)a.bands;
  const unsigned int plane = q % (unsigned int)a.planes, j = q / (unsigned int)a.planes;
  const int r0 = (int)band_i * a.band, r1 = min(a.Hout, r0 + a.band), nout = r1 - r0;
  const bool horiz = a.xbounds != nullptr, vert = a.ybounds != nullptr;

  // LDS: source rows | horizontal result | x bounds, x coefficients | y bounds, y coefficients (of this band)
  unsigned char* src = lds;
  unsigned char* mid = src + (((size_t)a.maxrows * a.SW + 15u) & ~(size_t)15u);
  int* xb = reinterpret_cast<int*>(mid + (horiz ? (((size_t)a.maxrows * a.MW + 15u) & ~(size_t)15u) : 0u));
  int* xc = xb + (horiz ? 2 * a.Wout : 0);
  int* yb = xc + (horiz ? a.Wout * a.kx : 0);
  int* yc = yb + (vert ? 2 * a.band : 0);

  const long long id = a.idx != nullptr ? a.idx[j] : (long long)j;
  int ylo = r0, yhi = r1;
  if (vert) {
    ylo = a.ybounds[2 * r0];
    yhi = a.ybounds[2 * (r1 - 1)] + a.ybounds[2 * (r1 - 1) + 1];
  }
  const int nrows = yhi - ylo;
  int fl = 0;
  if (id < 0 || id >= a.num_images)
    fl = 1;                                                    // as itcv_gather_u8: a zero image and bit 0
  else if (ylo < 0 || yhi > a.Hin || nrows < 1 || nrows > a.maxrows)
    fl = 2;                                                    // a plan that is not one of this shape: nothing is read
  const bool bad = fl != 0;
  if (bad && tid == 0 && (fl == 2 || (band_i == 0 && plane == 0))) atomicOr(a.flags, fl);

  if (!bad) {                                                  // block-uniform
    const unsigned char* g = a.table + ((size_t)id * a.planes + plane) * ((size_t)a.Hin * a.Win) + (size_t)ylo * a.Win;
    if (a.vec_in) {                                            // Win % 16 == 0: SW == Win, the rows are one aligned run
      const uint4* g4 = reinterpret_cast<const uint4*>(g);
      uint4* s4 = reinterpret_cast<uint4*>(src);
      const int n16 = (nrows * a.Win) >> 4;
      for (int i = tid; i < n16; i += 256) s4[i] = g4[i];
    } else {
      const int lw = 1 << a.lw_in, tx = tid & (lw - 1), ty = tid >> a.lw_in, rs = 256 >> a.lw_in;
      for (int row = ty; row < nrows; row += rs)
        for (int x = tx; x < a.Win; x += lw) src[row * a.SW + x] = g[(size_t)row * a.Win + x];
    }
    // plans, clamped to the arrays they index (a well-formed plan is unchanged by this)
    if (horiz) {
      for (int i = tid; i < a.Wout; i += 256) {
        int mn = a.xbounds[2 * i], c = a.xbounds[2 * i + 1];
        mn = min(max(mn, 0), a.Win);
        c = min(max(c, 0), min(a.kx, a.Win - mn));
        xb[2 * i] = mn, xb[2 * i + 1] = c;
      }
      for (int i = tid; i < a.Wout * a.kx; i += 256) xc[i] = a.xcoef[i];
    }
    if (vert) {
      for (int i = tid; i < nout; i += 256) {
        int mn = a.ybounds[2 * (r0 + i)] - ylo, c = a.ybounds[2 * (r0 + i) + 1];
        mn = min(max(mn, 0), nrows);
        c = min(max(c, 0), min(a.ky, nrows - mn));
        yb[2 * i] = mn, yb[2 * i + 1] = c;
      }
      for (int i = tid; i < nout * a.ky; i += 256) yc[i] = a.ycoef[(size_t)r0 * a.ky + i];
    }
    __syncthreads();

    if (horiz) {      // lane <-> output column; four source rows a step, so that a coefficient is read once for four
      const int lw = 1 << a.lw_out, tx = tid & (lw - 1), ty = tid >> a.lw_out, rs = 256 >> a.lw_out;
      for (int xx = tx; xx < a.Wout; xx += lw) {
        const int mn = xb[2 * xx], c = xb[2 * xx + 1];
        const int* kc = xc + xx * a.kx;
        for (int row = ty; row < nrows; row += 4 * rs) {
          const int last = nrows - 1;
          const unsigned char* s0 = src + row * a.SW + mn;
          const unsigned char* s1 = src + min(row + rs, last) * a.SW + mn;
          const unsigned char* s2 = src + min(row + 2 * rs, last) * a.SW + mn;
          const unsigned char* s3 = src + min(row + 3 * rs, last) * a.SW + mn;
          int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
          for (int t = 0; t < c; ++t) {
            const int k = kc[t];
            a0 += (int)s0[t] * k;
            a1 += (int)s1[t] * k;
            a2 += (int)s2[t] * k;
            a3 += (int)s3[t] * k;
          }
          unsigned char* m = mid + row * a.MW + xx;
          m[0] = (unsigned char)to_byte(a0);
          if (row + rs < nrows) m[rs * a.MW] = (unsigned char)to_byte(a1);
          if (row + 2 * rs < nrows) m[2 * rs * a.MW] = (unsigned char)to_byte(a2);
          if (row + 3 * rs < nrows) m[3 * rs * a.MW] = (unsigned char)to_byte(a3);
        }
      }
      __syncthreads();
    }
  }

  // vertical pass (or the copy out of LDS when the height does not change): lane <-> four neighbouring columns
  const unsigned char* rows = horiz ? mid : src;               // row stride MW either way: SW == MW when Win == Wout
  const bool mirrored = a.flip != nullptr && a.flip[j] != 0;
  const size_t plane_out = ((size_t)j * a.planes + plane) * ((size_t)a.Hout * a.Wout);
  const int quads = a.MW >> 2;
  const int lw = 1 << a.lw_quad, tx = tid & (lw - 1), ty = tid >> a.lw_quad, rs = 256 >> a.lw_quad;
  for (int r = ty; r < nout; r += rs) {
    const size_t o = plane_out + (size_t)(r0 + r) * a.Wout;
    for (int qd = tx; qd < quads; qd += lw) {
      int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
      if (!bad) {
        if (vert) {
          const int mn = yb[2 * r], c = yb[2 * r + 1];
          const int* kc = yc + r * a.ky;
          const unsigned char* p = rows + mn * a.MW + 4 * qd;
          int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
          for (int t = 0; t < c; ++t) {
            const unsigned int w = *reinterpret_cast<const unsigned int*>(p + t * a.MW);
            const int k = kc[t];
            a0 += (int)(w & 0xffu) * k;
            a1 += (int)((w >> 8) & 0xffu) * k;
            a2 += (int)((w >> 16) & 0xffu) * k;
            a3 += (int)(w >> 24) * k;
          }
          v0 = to_byte(a0), v1 = to_byte(a1), v2 = to_byte(a2), v3 = to_byte(a3);
        } else {
          const unsigned int w = *reinterpret_cast<const unsigned int*>(rows + r * a.MW + 4 * qd);
          v0 = (int)(w & 0xffu), v1 = (int)((w >> 8) & 0xffu), v2 = (int)((w >> 16) & 0xffu), v3 = (int)(w >> 24);
        }
      }
      const int x0 = 4 * qd;
      if (a.vec_out) {                                         // Wout % 4 == 0: a mirrored quad is a quad again
        if (mirrored) {
          const int t0 = v0, t1 = v1;
          v0 = v3, v1 = v2, v2 = t1, v3 = t0;
        }
        const int xd = mirrored ? a.Wout - 4 - x0 : x0;
        if constexpr (F32) {
          *reinterpret_cast<float4*>(static_cast<float*>(a.out) + o + xd) =
              make_float4((float)v0 / 255.0f, (float)v1 / 255.0f, (float)v2 / 255.0f, (float)v3 / 255.0f);
        } else {
          *reinterpret_cast<unsigned int*>(static_cast<unsigned char*>(a.out) + o + xd) =
              (unsigned int)v0 | ((unsigned int)v1 << 8) | ((unsigned int)v2 << 16) | ((unsigned int)v3 << 24);
        }
      } else {
        const int v[4] = {v0, v1, v2, v3};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int x = x0 + e;
          if (x < a.Wout) {
            const int xd = mirrored ? a.Wout - 1 - x : x;
            if constexpr (F32)
              static_cast<float*>(a.out)[o + xd] = (float)v[e] / 255.0f;
            else
              static_cast<unsigned char*>(a.out)[o + xd] = (unsigned char)v[e];
          }
        }
      }
    }
  }
}

// log2 of the lanes of a 256-thread block that walk one row of `width` items (the rest of the block takes other rows)
inline int lane_log2(int width) {
  int l = 0;
  while (l < 8 && (1 << l) < width) ++l;
  return l;
}

constexpr size_t kResizeLdsTarget = 64u << 10, kResizeLdsLimit = 160u << 10;

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_resize_u8(const unsigned char* table, long long num_images, int planes, int Hin, int Win, const long long* idx,
                   int n, const unsigned char* flip, const int* xbounds, const int* xcoef, int kx, const int* ybounds,
                   const int* ycoef, int ky, int Hout, int Wout, void* out, int out_is_f32, int* flags, void* stream) {
  const char* name = "itcv_resize_u8";
  ITCV_REQUIRE(table && out && flags, name);
  ITCV_REQUIRE(num_images > 0 && planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && n > 0, name);
  ITCV_REQUIRE((long long)planes * Hin * Win < (1ll << 31) && (long long)planes * Hout * Wout < (1ll << 31), name);
  ITCV_REQUIRE(idx != nullptr || n <= num_images, name);
  const bool horiz = xbounds != nullptr, vert = ybounds != nullptr;
  ITCV_REQUIRE(horiz ? (xcoef != nullptr && kx > 0) : (xcoef == nullptr && Wout == Win), name);
  ITCV_REQUIRE(vert ? (ycoef != nullptr && ky > 0) : (ycoef == nullptr && Hout == Hin), name);
  ITCV_REQUIRE(horiz || vert || !out_is_f32, name);          // a plain fp32 gather is itcv_gather_u8
  ITCV_REQUIRE(!horiz || (long long)Wout * kx < (1ll << 24), name);
  ITCV_REQUIRE(!vert || (long long)Hout * ky < (1ll << 24), name);

  ResizeArgs a;
  a.table = table, a.num_images = num_images, a.planes = planes, a.Hin = Hin, a.Win = Win, a.idx = idx, a.flip = flip;
  a.xbounds = xbounds, a.xcoef = xcoef, a.kx = horiz ? kx : 0, a.ybounds = ybounds, a.ycoef = ycoef, a.ky = vert ? ky : 0;
  a.Hout = Hout, a.Wout = Wout, a.out = out, a.flags = flags;
  a.SW = (int)align_up((size_t)Win, 4), a.MW = (int)align_up((size_t)Wout, 4);
  // a band of b output rows reads at most floor((b - 1) * Hin / Hout) + ky source rows (hipvae/resize.py: the first
  // and last windows are 2 * support + 1 <= ky wide and their centres (b - 1) * Hin / Hout apart); one row of slack
  auto rows_of = [&](int b) {
    const long long r = vert ? ((long long)(b - 1) * Hin) / Hout + ky + 1 : (long long)b;
    return (int)(r < Hin ? r : Hin);
  };
  auto lds_of = [&](int b) {
    const size_t rows = (size_t)rows_of(b);
    size_t s = align_up(rows * a.SW, 16);
    if (horiz) s += align_up(rows * a.MW, 16) + (size_t)Wout * (2 + kx) * sizeof(int);
    if (vert) s += (size_t)b * (2 + ky) * sizeof(int);
    return s;
  };
  int band = Hout;
  while (band > 1 && lds_of(band) > kResizeLdsTarget) band = (band + 1) / 2;
  ITCV_REQUIRE(lds_of(band) <= kResizeLdsLimit, name);
  // two blocks for each of the 256 CUs before bands grow tall (a short band recomputes more shared rows)
  while (band > 8 && (long long)n * planes * cdiv(Hout, band) < 512) band = (band + 1) / 2;
  a.band = band, a.bands = cdiv(Hout, band), a.maxrows = rows_of(band);
  const long long blocks = (long long)n * planes * a.bands;
  ITCV_REQUIRE(blocks < (1ll << 31), name);
  a.lw_in = lane_log2(Win), a.lw_out = lane_log2(Wout), a.lw_quad = lane_log2(a.MW / 4);
  a.vec_in = Win % 16 == 0 && (reinterpret_cast<uintptr_t>(table) & 15u) == 0;
  a.vec_out = Wout % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (out_is_f32 ? 15u : 3u)) == 0;
  const size_t lds = lds_of(band);
  if (out_is_f32)
    launch_lds<resize_u8_kernel<true>>(dim3((unsigned int)blocks), dim3(256), lds, S(stream), a);
  else
    launch_lds<resize_u8_kernel<false>>(dim3((unsigned int)blocks), dim3(256), lds, S(stream), a);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
