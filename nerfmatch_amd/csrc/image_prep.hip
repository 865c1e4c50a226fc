// Pillow-exact Lanczos resize of 8-bit images on the device (image_prep.py).  The reference resizes every image on the host with
// PIL.Image.resize(img_wh, Image.LANCZOS) (process_img, nerfmatch/datasets/nerfmatch_dataset.py:36-61 and nerfbase.py:197-237).  Pillow's
// 8-bit resampler is integer arithmetic on fixed-point coefficients with 22 fractional bits: a horizontal pass whose result is rounded and
// clipped to uint8, then a vertical pass over those bytes.  The coefficient tables come from the host (image_prep.lanczos_tables: float64,
// the C library's sin); the kernel sees integers only and reproduces every output byte.
//
// One launch for all F frames, one workgroup per tile of IMG_TW x IMG_TH output pixels:
//
//   1. The tile's source rows [ys, ye) -- the union of its output rows' vertical windows -- are taken in chunks of `stage_rows` rows.  A
//      chunk's bytes [xs C, xe C) (the union of the horizontal windows) are read from global memory once, in aligned 16-byte pieces, into
//      LDS; a row keeps its offset inside the first piece, so no lane ever loads single bytes of interleaved RGB from memory.
//   2. Horizontal pass on the chunk: lane = output column, wavefront w = rows w, w + 4, ... of the chunk.  One coefficient load (tap-major
//      table: consecutive lanes, consecutive words) feeds four rows x C channels.  The rounded, clipped bytes go to the `inter` array in
//      LDS, [row][IMG_TW][C]: the horizontally filtered rows never exist in global memory.
//   3. Vertical pass from `inter`: one thread makes four consecutive bytes of an output row from one 32-bit LDS word per tap.
//   4. Epilogue on the finished tile in LDS: white_where (255 in every channel where the operand is >= 128), the uint8 output as 32-bit
//      words where the row is aligned, the float output through the C x 256 look-up table as planes with the column in the lane.
//
// A pass whose axis keeps its size (ksize 0) runs as the one-tap window {i} with the coefficient 2^22, for which the fixed-point
// expression (2^21 + 2^22 v) >> 22 returns v: one code path.
//
// LDS: inter = rows x IMG_TW x C bytes with rows <= (IMG_TH - 1) scale + 6 max(scale, 1) + 1, the stage = stage_rows x pitch (the
// finished tile re-uses it), and the tile's coefficients where they fit.  The entry point sizes all of it inside 64 KiB, so two
// workgroups fit a compute unit at the largest supported reduction (8 x, C = 3: 297 rows = 57 KB + 5 staged rows, coefficients from the
// tables) and four at the shipped Cambridge ratio (84 rows = 16 KB + 16 staged rows = 13 KB + 8 KB of coefficients).
//
// Nothing a table holds can make the kernel leave the source or the LDS arrays: every window is clamped into the tile's span and the span
// into the image.  All arithmetic is int32, as in Pillow; the products are 24-bit multiplies (v_mad_i32_i24, four times the rate of the
// full 32-bit multiply): |coefficient| < 2^23 and a byte fit the signed 24-bit operands, and the entry point's ksize check keeps a table
// of another axis out.
#include "common.h"

namespace {

constexpr int IMG_TW = NM_IMAGE_TILE_W, IMG_TH = NM_IMAGE_TILE_H;
constexpr int IMG_THREADS = 256;
constexpr int IMG_ROWS_PER_WAVE = 4;                                     // horizontal pass: rows of a chunk per wavefront
constexpr int IMG_MAX_STAGE_ROWS = (IMG_THREADS / 64) * IMG_ROWS_PER_WAVE;  // 16
constexpr int IMG_LOADS = 4;                                             // staging: 16-byte loads of a thread in flight together
constexpr int IMG_MAX_SIDE = 8192;
constexpr int IMG_MAX_REDUCTION = 8;
constexpr int IMG_MAX_KSIZE = 51;  // the stated limit; 8 x gives ceil(3 * 8) * 2 + 1 = 49
constexpr int IMG_LDS_BYTES = 64 * 1024;
constexpr int IMG_ONE = 1 << 22;  // 1.0 in Pillow's fixed point (PRECISION_BITS = 32 - 8 - 2)

static_assert(IMG_TW == 64, "the horizontal pass puts one output column in each lane of a wavefront");
static_assert(IMG_TH * IMG_TW % IMG_THREADS == 0 && (IMG_TW % 4) == 0, "tile passes run in whole rounds of the workgroup");

struct ResizeArgs {
  const uint8_t* src;
  size_t src_bytes;
  int H, W, h, w;
  const int* coef_x;    // [ksize_x][w]  tap-major
  const int* bounds_x;  // [w][2] = first source column, number of taps
  const int* coef_y;    // [h][ksize_y]
  const int* bounds_y;  // [h][2]
  int ksize_x, ksize_y;
  const uint8_t* white;  // [F][h][w] or NULL
  const float* lut;      // [C][256]
  uint8_t* out_u8;       // [F][h][w][C] or NULL
  float* out_f32;        // [F][C][h][w] or NULL
  int max_rows, max_cols;  // bounds of a tile's source span: the sizes of `inter` and of a staged row
  int pitch, stage_rows;   // bytes of a staged row (a multiple of 16), rows per chunk (1 .. 16)
  int inter_bytes;         // offset of the stage behind `inter`
  int coef_off;            // offset of the tile's coefficient copies in LDS, or 0: the passes read the tables from global memory
};

// window of output i of one axis: first source index and number of taps (ksize 0: the identity pass)
__device__ __forceinline__ void img_window(const int* __restrict__ bounds, int ksize, int i, int& lo, int& n) {
  if (ksize) {
    lo = bounds[2 * i];
    n = min(bounds[2 * i + 1], ksize);
  } else {
    lo = i;
    n = 1;
  }
}

// Pillow's clip8: the accumulator starts at 2^21, is shifted arithmetically by 22 and clipped to [0, 255].  Written as clamp-then-shift
// (the same value: s < 0 -> 0, s >= 256 * 2^22 -> 255).  The shift-then-clamp form of two neighbouring bytes is folded by hipcc into one
// v_ashr_pk_u8_i32, whose result the vertical pass's byte packing then ORs into a word as if its upper half were zero; on gfx950 that
// half held bits of the first operand and bytes 2 and 3 of every word came out wrong.
__device__ __forceinline__ uint32_t img_clip8(int acc) {
  const int s = min(max(acc + (IMG_ONE >> 1), 0), 256 * IMG_ONE - 1);
  return (uint32_t)s >> 22;
}

template <int C>
__global__ void __launch_bounds__(IMG_THREADS) image_resize_u8_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int ROWB = IMG_TW * C;  // bytes of a tile row in `inter` and in the finished tile
  constexpr int DW = ROWB / 4;      // ... in 32-bit words
  uint8_t* inter = lds;
  uint8_t* stage = lds + a.inter_bytes;
  uint8_t* otile = stage;  // the finished tile: written after the last chunk has been consumed
  const int tid = threadIdx.x, f = blockIdx.z;
  const int tx0 = blockIdx.x * IMG_TW, ty0 = blockIdx.y * IMG_TH;
  const int tw = min(IMG_TW, a.w - tx0), th = min(IMG_TH, a.h - ty0);

  // the tile's source span; windows start and end in ascending order along an axis, so the first and the last one bound it
  int xs, xe, ys, ye, n_first, n_last;
  img_window(a.bounds_x, a.ksize_x, tx0, xs, n_first);
  img_window(a.bounds_x, a.ksize_x, tx0 + tw - 1, xe, n_last);
  xs = min(max(xs, 0), a.W - 1);
  xe = max(xe + n_last, xs + n_first);
  const int ncols = max(min(min(xe - xs, a.max_cols), a.W - xs), 1);
  img_window(a.bounds_y, a.ksize_y, ty0, ys, n_first);
  img_window(a.bounds_y, a.ksize_y, ty0 + th - 1, ye, n_last);
  ys = min(max(ys, 0), a.H - 1);
  ye = max(ye + n_last, ys + n_first);
  const int nrows = max(min(min(ye - ys, a.max_rows), a.H - ys), 1);

  // this lane's horizontal window, relative to the staged span
  const int xx = tid & 63, wave = tid >> 6;
  int rel_x = 0, n_x = 0;
  if (xx < tw) {
    int lo;
    img_window(a.bounds_x, a.ksize_x, tx0 + xx, lo, n_x);
    rel_x = min(max(lo - xs, 0), ncols - 1);
    n_x = max(min(n_x, ncols - rel_x), 0);
  }
  // the tile's coefficients: [ksize_x][IMG_TW] and [IMG_TH][ksize_y] words in LDS when the entry point found room for them.  A tap's
  // coefficient is then an LDS read; from the table it is a dependent load of L2 latency in front of every tap of every chunk.
  int* cxs = reinterpret_cast<int*>(lds + a.coef_off);
  int* cys = cxs + a.ksize_x * IMG_TW;
  if (a.coef_off) {
    for (int i = tid; i < a.ksize_x * IMG_TW; i += IMG_THREADS) {
      const int col = tx0 + (i & (IMG_TW - 1));
      cxs[i] = col < a.w ? a.coef_x[(size_t)(i / IMG_TW) * a.w + col] : 0;
    }
    for (int i = tid; i < th * a.ksize_y; i += IMG_THREADS) cys[i] = a.coef_y[(size_t)ty0 * a.ksize_y + i];
  }  // (visible to the passes behind the first chunk's barrier)

  const int ppr = a.pitch >> 4;  // 16-byte pieces of a staged row
  for (int r0 = 0; r0 < nrows; r0 += a.stage_rows) {
    const int rc = min(a.stage_rows, nrows - r0);
    // 1. source rows ys + r0 .. + rc, bytes [xs C, (xs + ncols) C), as the aligned 16-byte pieces that cover them; four loads of a
    //    thread are in flight together
    for (int base = 0; base < rc * ppr; base += IMG_LOADS * IMG_THREADS) {
      u32x4 v[IMG_LOADS];
      int dst[IMG_LOADS];
#pragma unroll
      for (int u = 0; u < IMG_LOADS; ++u) {
        const int i = base + u * IMG_THREADS + tid;
        const int r = i / ppr, piece = i - r * ppr;
        const size_t g0 = ((size_t)(f * (size_t)a.H + ys + r0 + min(r, rc - 1)) * a.W + xs) * C;
        const int shift = (int)(g0 & 15);
        const size_t at = g0 - shift + (size_t)piece * 16;
        dst[u] = (i < rc * ppr && piece * 16 < shift + ncols * C) ? r * a.pitch + piece * 16 : -1;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (dst[u] >= 0) {
          if (at + 16 <= a.src_bytes) {
            v[u] = *reinterpret_cast<const u32x4*>(a.src + at);
          } else {  // the last piece of the whole source, when its size is no multiple of 16
            for (int b = 0; b < 16; ++b)
              if (at + b < a.src_bytes) v[u][b >> 2] |= (uint32_t)a.src[at + b] << (8 * (b & 3));
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IMG_LOADS; ++u)
        if (dst[u] >= 0) *reinterpret_cast<u32x4*>(stage + dst[u]) = v[u];
    }
    __syncthreads();
    // 2. horizontal pass: rows wave, wave + 4, ... of the chunk (a row past the chunk re-reads its last row and is not written)
    if (n_x > 0) {
      // volatile: three byte reads per pixel stay three byte reads.  Merged into a 16-bit LDS read at an odd address (what hipcc makes of
      // them otherwise) they were several times slower on gfx950: C = 3 cost six times C = 1 for three times the bytes.
      const volatile uint8_t* rowp[IMG_ROWS_PER_WAVE];
      int acc[IMG_ROWS_PER_WAVE][C];
#pragma unroll
      for (int i = 0; i < IMG_ROWS_PER_WAVE; ++i) {
        const int r = min(wave + 4 * i, rc - 1);
        const size_t g0 = ((size_t)(f * (size_t)a.H + ys + r0 + r) * a.W + xs) * C;
        rowp[i] = stage + r * a.pitch + (int)(g0 & 15) + rel_x * C;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[i][c] = 0;
      }
      auto taps = [&](const int* __restrict__ coef, int stride) {
        for (int x = 0; x < n_x; ++x) {
          const int k = a.ksize_x ? coef[(size_t)x * stride] : IMG_ONE;
#pragma unroll
          for (int i = 0; i < IMG_ROWS_PER_WAVE; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][c] += __mul24(k, (int)rowp[i][x * C + c]);
        }
      };
      if (a.coef_off)
        taps(cxs + xx, IMG_TW);
      else
        taps(a.coef_x + tx0 + xx, a.w);
#pragma unroll
      for (int i = 0; i < IMG_ROWS_PER_WAVE; ++i) {
        const int r = wave + 4 * i;
        if (r < rc) {
#pragma unroll
          for (int c = 0; c < C; ++c) inter[(r0 + r) * ROWB + xx * C + c] = (uint8_t)img_clip8(acc[i][c]);
        }
      }
    }
    __syncthreads();  // the next chunk (or the finished tile) overwrites the stage
  }

  // 3. vertical pass: four consecutive bytes of an output row per thread (columns past tw hold arbitrary bytes and are never stored)
  const uint32_t* inter32 = reinterpret_cast<const uint32_t*>(inter);
  uint32_t* otile32 = reinterpret_cast<uint32_t*>(otile);
  for (int j = tid; j < IMG_TH * DW; j += IMG_THREADS) {
    const int yy = j / DW, d = j - yy * DW;
    if (yy >= th) continue;
    int lo, n;
    img_window(a.bounds_y, a.ksize_y, ty0 + yy, lo, n);
    const int rel = min(max(lo - ys, 0), nrows - 1);
    n = max(min(n, nrows - rel), 0);
    const int* __restrict__ cy = a.coef_off ? cys + yy * a.ksize_y : a.coef_y + (size_t)(ty0 + yy) * a.ksize_y;
    int acc[4] = {0, 0, 0, 0};
    for (int y = 0; y < n; ++y) {
      const int k = a.ksize_y ? cy[y] : IMG_ONE;
      const uint32_t word = inter32[(rel + y) * DW + d];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] += __mul24(k, (int)((word >> (8 * b)) & 255u));
    }
    otile32[yy * DW + d] = (uint32_t)img_clip8(acc[0]) | ((uint32_t)img_clip8(acc[1]) << 8) | ((uint32_t)img_clip8(acc[2]) << 16) |
                           ((uint32_t)img_clip8(acc[3]) << 24);
  }
  __syncthreads();

  // 4. epilogue.  `inter` is free now and takes the look-up table (inter_bytes >= C * 1024).
  float* lut_s = reinterpret_cast<float*>(inter);
  if (a.out_f32)
    for (int i = tid; i < C * 256; i += IMG_THREADS) lut_s[i] = a.lut[i];
  if (a.white) {
    for (int j = tid; j < IMG_TH * IMG_TW; j += IMG_THREADS) {
      const int yy = j / IMG_TW, px = j - yy * IMG_TW;
      if (yy < th && px < tw && a.white[((size_t)f * a.h + ty0 + yy) * a.w + tx0 + px] >= 128) {
#pragma unroll
        for (int c = 0; c < C; ++c) otile[yy * ROWB + px * C + c] = 255;
      }
    }
  }
  __syncthreads();
  if (a.out_u8) {
    const int nb = tw * C;  // bytes of a tile row that exist in the output
    for (int j = tid; j < IMG_TH * DW; j += IMG_THREADS) {
      const int yy = j / DW, b0 = 4 * (j - yy * DW);
      if (yy >= th || b0 >= nb) continue;
      const size_t ob = (((size_t)f * a.h + ty0 + yy) * a.w + tx0) * C + b0;  // (out_u8 itself is 16-byte aligned)
      if (!(ob & 3) && b0 + 4 <= nb) {
        *reinterpret_cast<uint32_t*>(a.out_u8 + ob) = otile32[j];
      } else {
        for (int b = 0; b < 4 && b0 + b < nb; ++b) a.out_u8[ob + b] = otile[yy * ROWB + b0 + b];
      }
    }
  }
  if (a.out_f32) {
    for (int j = tid; j < C * IMG_TH * IMG_TW; j += IMG_THREADS) {
      const int px = j % IMG_TW, yy = (j / IMG_TW) % IMG_TH, c = j / (IMG_TW * IMG_TH);
      if (yy < th && px < tw)
        a.out_f32[(((size_t)f * C + c) * a.h + ty0 + yy) * a.w + tx0 + px] = lut_s[c * 256 + otile[yy * ROWB + px * C + c]];
    }
  }
}

// Pillow's kernel size of one axis: ceil(3 max(in / out, 1)) * 2 + 1
int img_ksize(int in, int out) {
  const double scale = (double)in / out;
  return (int)__builtin_ceil(3.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

// upper bound of the source span of `tile` consecutive outputs: the first window starts above c - s - 1/2, the last one ends below
// c' + s + 1/2 with c' - c = (tile - 1) scale and s = 3 max(scale, 1)
int img_span(int in, int out, int ksize, int tile) {
  if (!ksize) return tile < in ? tile : in;
  const double scale = (double)in / out;
  const int span = (int)((tile - 1) * scale + 6.0 * (scale < 1.0 ? 1.0 : scale) + 1.0);
  return span < in ? span : in;
}

}  // namespace

extern "C" int nm_image_resize_u8(const uint8_t* src, int F, int H, int W, int C, const int* coef_x, const int* bounds_x, int ksize_x,
                                  const int* coef_y, const int* bounds_y, int ksize_y, int h, int w, const uint8_t* white_where,
                                  const float* lut, uint8_t* out_u8, float* out_f32, nmStream_t stream) {
  NM_CHECK_ARG(src && F > 0 && H > 0 && W > 0 && h > 0 && w > 0 && (out_u8 || out_f32) && (!out_f32 || lut));
  NM_CHECK_ARG(ksize_x >= 0 && ksize_y >= 0 && (ksize_x ? (coef_x && bounds_x) : W == w) && (ksize_y ? (coef_y && bounds_y) : H == h));
  NM_CHECK_ARG((((uintptr_t)src | (uintptr_t)out_u8 | (uintptr_t)out_f32) & 15) == 0);
  if ((C != 1 && C != 3) || F > 65535 || H > IMG_MAX_SIDE || W > IMG_MAX_SIDE || h > IMG_MAX_SIDE || w > IMG_MAX_SIDE) return NM_ERR_UNSUPPORTED;
  if (W > IMG_MAX_REDUCTION * (long long)w || H > IMG_MAX_REDUCTION * (long long)h || ksize_x > IMG_MAX_KSIZE || ksize_y > IMG_MAX_KSIZE)
    return NM_ERR_UNSUPPORTED;
  NM_CHECK_ARG((!ksize_x || ksize_x == img_ksize(W, w)) && (!ksize_y || ksize_y == img_ksize(H, h)));
  ResizeArgs a;
  a.src = src;
  a.src_bytes = (size_t)F * H * W * C;
  a.H = H, a.W = W, a.h = h, a.w = w;
  a.coef_x = coef_x, a.bounds_x = bounds_x, a.coef_y = coef_y, a.bounds_y = bounds_y;
  a.ksize_x = ksize_x, a.ksize_y = ksize_y;
  a.white = white_where, a.lut = lut, a.out_u8 = out_u8, a.out_f32 = out_f32;
  a.max_rows = img_span(H, h, ksize_y, IMG_TH);
  a.max_cols = img_span(W, w, ksize_x, IMG_TW);
  a.pitch = (15 + a.max_cols * C + 15) & ~15;
  const int row_bytes = IMG_TW * C, tile_bytes = IMG_TH * row_bytes;
  a.inter_bytes = a.max_rows * row_bytes;
  if (a.inter_bytes < C * 1024) a.inter_bytes = C * 1024;  // the epilogue's look-up table
  a.inter_bytes = (a.inter_bytes + 15) & ~15;
  // the tile's coefficients go to LDS too where they leave room for the finished tile and four staged rows (every shape but C = 3 near
  // the largest reduction)
  const int coef_bytes = (ksize_x * IMG_TW + IMG_TH * ksize_y) * (int)sizeof(int);
  int room = IMG_LDS_BYTES - a.inter_bytes;
  a.coef_off = 0;
  if (coef_bytes > 0 && room - coef_bytes >= tile_bytes && room - coef_bytes >= 4 * a.pitch) {
    room -= coef_bytes;
    a.coef_off = IMG_LDS_BYTES;  // (placed below, behind the stage)
  }
  a.stage_rows = room / a.pitch;
  if (a.stage_rows > IMG_MAX_STAGE_ROWS) a.stage_rows = IMG_MAX_STAGE_ROWS;
  if (a.stage_rows < 1 || room < tile_bytes) return NM_ERR_UNSUPPORTED;  // (not reached inside the limits above)
  int stage_bytes = a.stage_rows * a.pitch;
  if (stage_bytes < tile_bytes) stage_bytes = tile_bytes;
  const dim3 grid((w + IMG_TW - 1) / IMG_TW, (h + IMG_TH - 1) / IMG_TH, F);
  size_t lds = (size_t)a.inter_bytes + stage_bytes;
  if (a.coef_off) {
    a.coef_off = (int)lds;
    lds += coef_bytes;
  }
  if (C == 3)
    image_resize_u8_kernel<3><<<grid, IMG_THREADS, lds, (hipStream_t)stream>>>(a);
  else
    image_resize_u8_kernel<1><<<grid, IMG_THREADS, lds, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}
