// Audio conditioning front-end kernels: everything between a 16 kHz waveform and the token
// matrix the ImageBind audio ViT consumes.  They run once per clip; none is on the denoising loop.
//
// fbank_kernel: Kaldi-compatible log-mel filterbank, the algorithm torchaudio.compliance.kaldi.fbank runs for
//   ImageBind's waveform2melspec(htk_compat, hanning window, 25 ms / 10 ms frames, 128 bins, dither 0) followed
//   by the (mel, time) transpose, zero padding / cropping to `t_out` frames and the (x - mean) / std normalisation
//   of avgen/data/utils.py:26-55 (waveform_to_melspectrogram).  One workgroup per output frame: DC removal,
//   pre-emphasis, window, a direct 512-point DFT in f32 (400 x 257 complex MACs - 40 MFLOP per clip), power
//   spectrum, triangular mel filters, log.
// patchify_kernel: the non-overlapping-free 16x16 stride-10 patch gather in front of ImageBind's audio stem
//   (Conv2d(1, 768, 16, stride 10, bias=False) == im2col + GEMM), f32 image -> bf16 rows [B*ph*pw][C*kh*kw].
// tokens_kernel: token matrix = [cls | patch embeddings] + learned position table, in sequences padded by
//   `tail` extra rows (the add_bias_kv key/value slot of torch.nn.MultiheadAttention lives in the first one).
// resample_kernel: the polyphase windowed-sinc sample-rate converter in front of all of the above
//   (torchaudio.functional.resample: avgen/data/utils.py:259,404, compute_avsync.py:141,157).  The filter bank is built on
//   the host (asva_amd/audio_features.py:resample_taps); the kernel is a strided FIR, f32 FMA on the vector ALU - 15 MFLOP
//   per 2 s clip at 44.1 -> 16 kHz, launch-bound, so MFMA is not warranted.
#include "avsd_common.h"

namespace {

constexpr int FB_THREADS = 256;

struct FbankArgs {
  const float* wave; int64_t wave_stride; int n_samples;
  const float* window; const float* mel_fb;
  int win, shift, nfft, n_mel, n_frames;
  float preemph; int remove_dc;
  float* out; int t_out; float mean, inv_std;
};

__global__ __launch_bounds__(FB_THREADS) void fbank_kernel(const FbankArgs p) {
  extern __shared__ float fb_smem[];
  const int nbin = p.nfft / 2 + 1;
  float* x = fb_smem;                 // [nfft]   framed samples
  float* twc = x + p.nfft;            // [nfft]   cos(2 pi j / nfft)
  float* tws = twc + p.nfft;          // [nfft]   sin(2 pi j / nfft)
  float* pw = tws + p.nfft;           // [nbin]   power spectrum
  __shared__ float red[FB_THREADS / 64];

  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float* out = p.out + ((int64_t)b * p.n_mel) * p.t_out + t;
  if (t >= p.n_frames) {              // zero padding of the (un-normalised) log-mel matrix
    for (int m = tid; m < p.n_mel; m += FB_THREADS) out[(int64_t)m * p.t_out] = (0.f - p.mean) * p.inv_std;
    return;
  }
  const float* w = p.wave + (int64_t)b * p.wave_stride + (int64_t)t * p.shift;
  float part = 0.f;
  for (int i = tid; i < p.nfft; i += FB_THREADS) {
    const float v = i < p.win ? w[i] : 0.f;
    x[i] = v;
    part += v;
    float s, c;
    sincospif(2.0f * (float)i / (float)p.nfft, &s, &c);
    twc[i] = c;
    tws[i] = s;
  }
  part = wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  float mean = 0.f;
  if (p.remove_dc) {
    for (int i = 0; i < FB_THREADS / 64; ++i) mean += red[i];
    mean /= (float)p.win;
  }
  // pre-emphasis on the DC-free frame (Kaldi: x[i] -= c * x[i-1] from the back, x[0] -= c * x[0]), then window
  float y[2];
  int ny = 0;
  for (int i = tid; i < p.win; i += FB_THREADS) {
    const float cur = x[i] - mean;
    const float prev = x[i > 0 ? i - 1 : 0] - mean;
    y[ny++] = (cur - p.preemph * prev) * p.window[i];
  }
  __syncthreads();
  ny = 0;
  for (int i = tid; i < p.win; i += FB_THREADS) x[i] = y[ny++];
  __syncthreads();

  // direct DFT: bin k = sum_n x[n] * exp(-2 pi i k n / nfft)
  const int mask = p.nfft - 1;        // nfft is a power of two (host-checked)
  for (int k = tid; k < nbin; k += FB_THREADS) {
    float re = 0.f, im = 0.f;
    int j = 0;
    for (int n = 0; n < p.win; ++n) {
      const float v = x[n];
      re = fmaf(v, twc[j], re);
      im = fmaf(-v, tws[j], im);
      j = (j + k) & mask;
    }
    pw[k] = re * re + im * im;
  }
  __syncthreads();
  for (int m = tid; m < p.n_mel; m += FB_THREADS) {
    const float* f = p.mel_fb + (int64_t)m * nbin;
    float e = 0.f;
    for (int k = 0; k < nbin; ++k) e = fmaf(f[k], pw[k], e);
    e = logf(fmaxf(e, 1.1920928955078125e-07f));      // torch.finfo(float32).eps floor, as torchaudio
    out[(int64_t)m * p.t_out] = (e - p.mean) * p.inv_std;
  }
}

__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ src, h16_t* __restrict__ dst, int B, int C,
                                                       int H, int W, int kh, int kw, int stride, int ph, int pw_) {
  const int kk = C * kh * kw;
  const int64_t total = (int64_t)B * ph * pw_ * kk;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i % kk);
    const int64_t r = i / kk;
    const int px = (int)(r % pw_);
    const int py = (int)((r / pw_) % ph);
    const int b = (int)(r / ((int64_t)pw_ * ph));
    const int dx = e % kw, dy = (e / kw) % kh, c = e / (kw * kh);
    dst[i] = f2h(src[(((int64_t)b * C + c) * H + py * stride + dy) * W + px * stride + dx]);
  }
}

__global__ __launch_bounds__(256) void tokens_kernel(const h16_t* __restrict__ patches, const float* __restrict__ cls,
                                                     const float* __restrict__ pos, h16_t* __restrict__ out, int B, int np,
                                                     int C, int tail) {
  const int L = 1 + np + tail;
  const int64_t total = (int64_t)B * L * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int l = (int)((i / C) % L);
    const int b = (int)(i / ((int64_t)C * L));
    float v = 0.f;
    if (l == 0) v = cls[c] + pos[c];
    else if (l <= np) v = h2f(patches[((int64_t)b * np + (l - 1)) * C + c]) + pos[(int64_t)l * C + c];
    out[i] = f2h(v);
  }
}

// ---- sample-rate conversion ------------------------------------------------------------------------------------------
// out[w][q * new_ + p] = sum_k taps[p][k] * xpad(w, q * orig + k - width): the input window depends on q only, the filter row
// on p only.  Lanes run along q and a wave works on RS_PH phases at a time, so one LDS read of x feeds RS_PH FMAs and the
// filter taps are wave-uniform (one address per wave: they come through the scalar cache into SGPRs).  A workgroup of 4 waves covers 64 * WQ consecutive q
// (WQ waves along q, 4 / WQ waves along the phase) of one waveform and `phases` filter rows, and stages the
// 64 * WQ * orig + 2 * width samples that those q touch in LDS, writing the zero padding there.  STAGE = false reads the row
// directly, bounds-checked per sample: the path for decimation ratios whose window does not fit LDS.
// Every output is one k-ascending fmaf chain in one f32 accumulator, whatever the tile, grid or batch.
constexpr int RS_THREADS = 256;
constexpr int RS_PH = 4;                       // phases a wave accumulates at once
constexpr int RS_SB = 8;                       // staging loads a thread keeps in flight
constexpr size_t RS_LDS_MAX = 128 * 1024;      // of the 160 KiB; 44.1 -> 16 kHz needs 110.4 KiB at 64 q per workgroup

// xpad(s): the address is clamped into the row and the value replaced afterwards, so nothing outside [0, n_in) is read and the
// load is unconditional - a load under a per-element branch is waited for one element at a time
__device__ __forceinline__ float load_padded(const float* __restrict__ x, int64_t s, int n_in) {
  const int64_t c = s < 0 ? 0 : (s >= n_in ? (int64_t)n_in - 1 : s);
  const float v = x[c];
  return c == s ? v : 0.f;
}

struct ResampleArgs {
  int64_t x_stride; int n_in;
  int orig, new_, width, L;
  int64_t out_stride; int n_out;
  int nq, n_tiles, phases;                     // ceil(n_out / new_); q tiles per waveform; filter rows per workgroup
};

template <int WQ, bool STAGE>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ xg, const float* __restrict__ taps,
                                                              float* __restrict__ og, const ResampleArgs a) {
  extern __shared__ float rs_x[];              // [64 * WQ * orig + 2 * width]
  constexpr int QT = 64 * WQ, WP = RS_THREADS / QT;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = blockIdx.x / a.n_tiles, tile = blockIdx.x - w * a.n_tiles;
  const int q0 = tile * QT;
  const float* __restrict__ x = xg + (int64_t)w * a.x_stride;
  const int64_t base = (int64_t)q0 * a.orig - a.width;          // row index of rs_x[0]
  if constexpr (STAGE) {
    const int n_stage = QT * a.orig + 2 * a.width;
    for (int i0 = tid; i0 < n_stage; i0 += RS_THREADS * RS_SB) {      // RS_SB loads in flight per thread, then their LDS writes
      float v[RS_SB];
#pragma unroll
      for (int u = 0; u < RS_SB; ++u) v[u] = load_padded(x, base + i0 + u * RS_THREADS, a.n_in);
#pragma unroll
      for (int u = 0; u < RS_SB; ++u)
        if (i0 + u * RS_THREADS < n_stage) rs_x[i0 + u * RS_THREADS] = v[u];
    }
    __syncthreads();
  }
  const int ql = (wave % WQ) * 64 + (tid & 63);
  const int q = q0 + ql;
  if (q >= a.nq) return;                                        // after the only barrier
  const int p_begin = blockIdx.y * a.phases;
  const int p_end = min(p_begin + a.phases, a.new_);
  const float* xs = rs_x + ql * a.orig;
  const int64_t g0 = base + (int64_t)ql * a.orig;               // row index of this q's first tap
  float* __restrict__ out = og + (int64_t)w * a.out_stride;
  for (int p = p_begin + (wave / WQ) * RS_PH; p < p_end; p += WP * RS_PH) {
    const float* __restrict__ t[RS_PH];
#pragma unroll
    for (int j = 0; j < RS_PH; ++j) t[j] = taps + (int64_t)min(p + j, a.new_ - 1) * a.L;
    float acc[RS_PH] = {};
#pragma unroll 8
    for (int k = 0; k < a.L; ++k) {
      float v;
      if constexpr (STAGE) {
        v = xs[k];
      } else {
        v = load_padded(x, g0 + k, a.n_in);
      }
#pragma unroll
      for (int j = 0; j < RS_PH; ++j) acc[j] = fmaf(t[j][k], v, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < RS_PH; ++j) {
      const int64_t o = (int64_t)q * a.new_ + p + j;
      if (p + j < p_end && o < a.n_out) out[o] = acc[j];
    }
  }
}

template <int WQ, bool STAGE>
int launch_resample(const float* x, const float* taps, float* out, const ResampleArgs& a, size_t lds, dim3 grid, hipStream_t s) {
  static bool attr_set = false;
  if (STAGE && !attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_kernel<WQ, STAGE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)RS_LDS_MAX);
    if (e != hipSuccess) {
      avsd_set_error("resample_sinc: hipFuncSetAttribute(%zu B LDS): %s", RS_LDS_MAX, hipGetErrorString(e));
      return AVSD_ELAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((resample_kernel<WQ, STAGE>), grid, dim3(RS_THREADS), STAGE ? lds : 0, s, x, taps, out, a);
  AVSD_CHECK_LAUNCH("resample_sinc launch");
  return AVSD_OK;
}

}  // namespace

extern "C" int avsd_kaldi_fbank(const float* wave, int batch, int n_samples, int64_t wave_stride, const float* window,
                                const float* mel_fb, int win, int shift, int nfft, int n_mel, float preemph, int remove_dc,
                                float* out, int t_out, float mean, float std, void* stream) {
  AVSD_REQUIRE(wave && window && mel_fb && out, "fbank: null pointer");
  AVSD_REQUIRE(batch > 0 && win > 0 && shift > 0 && n_mel > 0 && t_out > 0, "fbank: bad sizes");
  AVSD_REQUIRE(nfft >= win && (nfft & (nfft - 1)) == 0 && nfft <= 4096, "fbank: nfft (%d) must be a power of two >= win (%d)", nfft, win);
  AVSD_REQUIRE(win <= 2 * FB_THREADS, "fbank: window of %d samples exceeds %d", win, 2 * FB_THREADS);
  AVSD_REQUIRE(std > 0.f, "fbank: std must be positive");
  FbankArgs a;
  a.wave = wave; a.wave_stride = wave_stride; a.n_samples = n_samples; a.window = window; a.mel_fb = mel_fb;
  a.win = win; a.shift = shift; a.nfft = nfft; a.n_mel = n_mel;
  a.n_frames = n_samples < win ? 0 : 1 + (n_samples - win) / shift;      // snip_edges = True
  a.preemph = preemph; a.remove_dc = remove_dc; a.out = out; a.t_out = t_out; a.mean = mean; a.inv_std = 1.0f / std;
  const size_t lds = (size_t)(3 * nfft + nfft / 2 + 1) * sizeof(float);
  hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)t_out, (unsigned)batch), dim3(FB_THREADS), lds,
                     reinterpret_cast<hipStream_t>(stream), a);
  AVSD_CHECK_LAUNCH("fbank launch");
  return AVSD_OK;
}

extern "C" int avsd_resample_sinc_f32(const float* x, int n_wav, int n_in, int64_t x_stride, const float* taps, int orig, int new_,
                                      int width, float* out, int n_out, int64_t out_stride, void* stream) {
  AVSD_REQUIRE(x && taps && out, "resample_sinc: null pointer");
  AVSD_REQUIRE(n_wav > 0 && n_in > 0 && orig > 0 && new_ > 0 && width > 0 && n_out > 0, "resample_sinc: bad sizes");
  const int64_t L = 2 * (int64_t)width + orig;
  AVSD_REQUIRE((int64_t)new_ * L <= ((int64_t)1 << 24),
               "resample_sinc: a filter bank of %d x %lld taps exceeds 2^24 floats (rates %d : %d after dividing by their gcd)", new_,
               (long long)L, orig, new_);
  const int64_t want = ((int64_t)new_ * n_in + orig - 1) / orig;
  AVSD_REQUIRE((int64_t)n_out == want, "resample_sinc: n_out (%d) must be ceil(new * n_in / orig) = %lld", n_out, (long long)want);
  AVSD_REQUIRE(x_stride >= n_in && out_stride >= n_out, "resample_sinc: strides (%lld, %lld) shorter than the rows (%d, %d)",
               (long long)x_stride, (long long)out_stride, n_in, n_out);
  ResampleArgs a;
  a.x_stride = x_stride; a.n_in = n_in; a.orig = orig; a.new_ = new_; a.width = width; a.L = (int)L;
  a.out_stride = out_stride; a.n_out = n_out;
  a.nq = (int)(((int64_t)n_out + new_ - 1) / new_);
  // 256 q per workgroup where their window fits the default 64 KiB of LDS (48 -> 16 kHz has one phase, 8 -> 16 kHz two: all four
  // waves run along q), else 64 q and the four waves on different phases, else no staging
  const size_t lds256 = (256 * (size_t)orig + 2 * (size_t)width) * sizeof(float);
  const size_t lds64 = (64 * (size_t)orig + 2 * (size_t)width) * sizeof(float);
  const int wq = lds256 <= 64 * 1024 ? 4 : 1;
  const bool stage = wq == 4 || lds64 <= RS_LDS_MAX;
  const int qt = 64 * wq, wp = RS_THREADS / qt;
  a.n_tiles = (a.nq + qt - 1) / qt;
  a.phases = wp * RS_PH;                                          // one pass of the workgroup ...
  while (((int64_t)new_ + a.phases - 1) / a.phases > 65535) a.phases *= 2;   // ... unless grid.y would overflow
  const int64_t gx = (int64_t)n_wav * a.n_tiles;
  AVSD_REQUIRE(gx <= 0x7fffffffLL, "resample_sinc: %d waveforms x %d tiles exceed the grid", n_wav, a.n_tiles);
  const dim3 grid((unsigned)gx, (unsigned)((new_ + a.phases - 1) / a.phases));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (wq == 4) return launch_resample<4, true>(x, taps, out, a, lds256, grid, s);
  if (stage) return launch_resample<1, true>(x, taps, out, a, lds64, grid, s);
  return launch_resample<1, false>(x, taps, out, a, 0, grid, s);
}

extern "C" int avsd_patchify(const float* src, void* dst, int B, int C, int H, int W, int kh, int kw, int stride, void* stream) {
  AVSD_REQUIRE(src && dst, "patchify: null pointer");
  AVSD_REQUIRE(B > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && H >= kh && W >= kw, "patchify: bad sizes");
  const int ph = (H - kh) / stride + 1, pw = (W - kw) / stride + 1;
  const int64_t total = (int64_t)B * ph * pw * C * kh * kw;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
                     reinterpret_cast<h16_t*>(dst), B, C, H, W, kh, kw, stride, ph, pw);
  AVSD_CHECK_LAUNCH("patchify launch");
  return AVSD_OK;
}

extern "C" int avsd_vit_tokens(const void* patches, const float* cls, const float* pos, void* out, int B, int n_patches, int C,
                               int tail_rows, void* stream) {
  AVSD_REQUIRE(patches && cls && pos && out, "vit_tokens: null pointer");
  AVSD_REQUIRE(B > 0 && n_patches > 0 && C > 0 && tail_rows >= 0, "vit_tokens: bad sizes");
  const int64_t total = (int64_t)B * (1 + n_patches + tail_rows) * C;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(tokens_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const h16_t*>(patches), cls, pos, reinterpret_cast<h16_t*>(out), B, n_patches, C, tail_rows);
  AVSD_CHECK_LAUNCH("vit_tokens launch");
  return AVSD_OK;
}
