// Video-LLM connector (the reference's VideoQA tail, llava_arch: mm_projector at :213, get_2dPool at :171-190, the newline placement at
// :261-288 and :351-390): the vision tower's features [F, P * P, in_dim] -> the language model's input rows [tokens, out_dim].  The
// Linears run on the encoder's GEMM launchers (sf_launch_gemm, both compute modes, weights rounded / split ONCE at finalize); this
// file adds the one kernel the encoder never needed, the launch sequence and the C entry points.
//
//   sf_connector_pool_kernel   spatial pool + output layout, a pure streaming kernel.  One work item = 8 consecutive channels of one
//                              OUTPUT row: the row index decodes to (frame, cell) or to a newline row, the taps of the cell are read
//                              with 16-byte loads, combined in fp32 in one fixed order, and stored with 16-byte stores.  Two roles:
//                                (a) planes in, planes out: bf16 hi (+ lo) planes as SF_EPI_ACT_BF16 emits them, summed to fp32, pooled,
//                                    re-split into the A operand of the last Linear;
//                                (b) fp32 in, final sequence out: fp32 or bf16 (round-to-nearest-even) rows at their place in the
//                                    sequence, the image_newline rows in the same launch.
//                              No LDS, no atomics, every output element has one owner: bit-reproducible.  Grid: one item per thread, 64
//                              threads per workgroup while the call is small (one frame of 49 x 3584 outputs is 22 K items = 343
//                              workgroups, more than the 256 CUs), 256 threads and a grid-stride loop capped at 2048 workgroups above.
//
// Tap rules are PyTorch's.  bilinear (F.interpolate, align_corners=False, no antialias): P' = ceil(P / s), src = (dst + 0.5) (P / P') - 0.5
// clamped below at 0, i0 = floor(src), i1 = min(i0 + 1, P - 1), lambda = src - i0: 2 x 2 taps at every stride.  average / max
// (F.avg_pool2d / F.max_pool2d): P' = floor(P / s) over s x s windows, trailing rows and columns dropped.
//
// Schedule (sf_connector_forward): average and bilinear are linear maps over patch positions whose weights sum to 1, so they commute
// with the last Linear, pool(x W^T + b) = pool(x) W^T + b: the pool runs in role (a) in FRONT of the last GEMM, which then sees P'^2
// rows per frame instead of P^2, and role (b) only places rows.  max does not commute and keeps the reference's order.
#include "sf_handle.h"

typedef __attribute__((ext_vector_type(4))) float cf4_t;

enum { CONN_POOL_NONE = 0, CONN_POOL_AVERAGE = 1, CONN_POOL_MAX = 2, CONN_POOL_BILINEAR = 3 };
enum { CONN_NL_NONE = 0, CONN_NL_ONE = 1, CONN_NL_FRAME = 2, CONN_NL_GRID = 3 };

// ------------------------------------------------------------------------------------------------
// kernel
// ------------------------------------------------------------------------------------------------
struct SfConnPool {
  const float* in_f32;                      // [F, P * P, C]            (fp32 input form)
  const bf16_t* in_hi; const bf16_t* in_lo; // the same as bf16 planes  (plane input form; lo may be null)
  float* out_f32; bf16_t* out_bf16;         // OUT 0 / OUT 1
  bf16_t* out_hi; bf16_t* out_lo;           // OUT 2 (lo may be null)
  const float* newline;                     // [C], read only when nl != CONN_NL_NONE
  int F, P, Po, C, C8;                      // Po = P' (output cells per side), C8 = C / 8
  int mode, stride, nl;
  unsigned total;                           // output rows * C8
  float scale;                              // bilinear: (float)P / Po
};

template <bool PLANES>
SF_DEVICE void conn_load8(const SfConnPool& p, size_t e, float v[8]) {
  if (PLANES) {
    const u32x4_t h = *reinterpret_cast<const u32x4_t*>(p.in_hi + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(h[j] << 16); v[2 * j + 1] = __uint_as_float(h[j] & 0xffff0000u); }
    if (p.in_lo) {
      const u32x4_t l = *reinterpret_cast<const u32x4_t*>(p.in_lo + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[2 * j] += __uint_as_float(l[j] << 16); v[2 * j + 1] += __uint_as_float(l[j] & 0xffff0000u); }
    }
  } else {
    const cf4_t a = *reinterpret_cast<const cf4_t*>(p.in_f32 + e), b = *reinterpret_cast<const cf4_t*>(p.in_f32 + e + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
}

template <bool PLANES, int OUT>      // OUT: 0 fp32 rows, 1 bf16 rows, 2 bf16 hi (+ lo) planes
__global__ __launch_bounds__(256) void sf_connector_pool_kernel(SfConnPool p) {
  const int P = p.P, Po = p.Po;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += gridDim.x * blockDim.x) {
    const unsigned r = i / (unsigned)p.C8;
    const int c = (int)(i - r * (unsigned)p.C8) * 8;
    // ---- output row -> (frame, cell) or a newline row ----
    int f, oy, ox;
    bool newline = false;
    if (p.nl == CONN_NL_GRID) {
      const int per = Po * (Po + 1);
      f = (int)(r / (unsigned)per);
      const int rr = (int)(r - (unsigned)f * per);
      oy = rr / (Po + 1); ox = rr - oy * (Po + 1);
      newline = ox == Po;
    } else if (p.nl == CONN_NL_FRAME) {
      const int per = Po * Po + 1;
      f = (int)(r / (unsigned)per);
      const int rr = (int)(r - (unsigned)f * per);
      oy = rr / Po; ox = rr - oy * Po;
      newline = rr == Po * Po;
    } else {
      const int per = Po * Po;
      f = (int)(r / (unsigned)per);
      const int rr = (int)(r - (unsigned)f * per);
      oy = rr / Po; ox = rr - oy * Po;
      newline = f >= p.F;                      // CONN_NL_ONE: the one row past the last frame
    }
    float y[8];
    if (newline) {
      const cf4_t a = *reinterpret_cast<const cf4_t*>(p.newline + c), b = *reinterpret_cast<const cf4_t*>(p.newline + c + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { y[j] = a[j]; y[4 + j] = b[j]; }
    } else {
      const size_t fb = (size_t)f * P * P;
#define CONN_AT(yy, xx) ((fb + (size_t)(yy) * P + (xx)) * p.C + c)
      if (p.mode == CONN_POOL_NONE) {
        conn_load8<PLANES>(p, CONN_AT(oy, ox), y);
      } else if (p.mode == CONN_POOL_BILINEAR) {
        float sy = p.scale * ((float)oy + 0.5f) - 0.5f, sx = p.scale * ((float)ox + 0.5f) - 0.5f;
        sy = sy < 0.f ? 0.f : sy; sx = sx < 0.f ? 0.f : sx;
        int y0 = (int)sy, x0 = (int)sx;
        y0 = y0 > P - 1 ? P - 1 : y0; x0 = x0 > P - 1 ? P - 1 : x0;
        const int y1 = y0 + (y0 < P - 1 ? 1 : 0), x1 = x0 + (x0 < P - 1 ? 1 : 0);
        const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
        const float hy = 1.f - ly, hx = 1.f - lx;
        float v00[8], v01[8], v10[8], v11[8];
        conn_load8<PLANES>(p, CONN_AT(y0, x0), v00); conn_load8<PLANES>(p, CONN_AT(y0, x1), v01);
        conn_load8<PLANES>(p, CONN_AT(y1, x0), v10); conn_load8<PLANES>(p, CONN_AT(y1, x1), v11);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = hy * (hx * v00[j] + lx * v01[j]) + ly * (hx * v10[j] + lx * v11[j]);
      } else {
        const int s = p.stride;
        const bool is_max = p.mode == CONN_POOL_MAX;
        conn_load8<PLANES>(p, CONN_AT(oy * s, ox * s), y);
        for (int k = 1; k < s * s; ++k) {      // row-major over the window: one fixed order
          const int dy = k / s, dx = k - dy * s;
          float v[8];
          conn_load8<PLANES>(p, CONN_AT(oy * s + dy, ox * s + dx), v);
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] = is_max ? ((v[j] > y[j] || v[j] != v[j]) ? v[j] : y[j]) : y[j] + v[j];      // F.max_pool2d's rule: a NaN wins
        }
        if (!is_max) {
          const float div = (float)(s * s);
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] = y[j] / div;
        }
      }
#undef CONN_AT
    }
    const size_t o = (size_t)r * p.C + c;
    if (OUT == 0) {
      *reinterpret_cast<cf4_t*>(p.out_f32 + o) = (cf4_t){y[0], y[1], y[2], y[3]};
      *reinterpret_cast<cf4_t*>(p.out_f32 + o + 4) = (cf4_t){y[4], y[5], y[6], y[7]};
    } else if (OUT == 1) {
      *reinterpret_cast<u32x4_t*>(p.out_bf16 + o) = (u32x4_t){pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]), pack_bf2(y[4], y[5]), pack_bf2(y[6], y[7])};
    } else {
      store_planes8(y, p.out_hi, p.out_lo, o);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// geometry and launcher
// ------------------------------------------------------------------------------------------------
static int conn_out_side(int P, int mode, int stride) {
  if (mode == CONN_POOL_NONE || stride <= 1) return P;
  return mode == CONN_POOL_BILINEAR ? (P + stride - 1) / stride : P / stride;
}
static int64_t conn_rows(int F, int Po, int nl) {
  const int64_t cells = (int64_t)Po * Po;
  switch (nl) {
    case CONN_NL_ONE: return (int64_t)F * cells + 1;
    case CONN_NL_FRAME: return (int64_t)F * (cells + 1);
    case CONN_NL_GRID: return (int64_t)F * Po * (Po + 1);
    default: return (int64_t)F * cells;
  }
}

// every pointer 16-byte aligned, C % 8 == 0, rows * C and F * P * P * C below 2^31: checked by the callers (conn_pool_check)
static hipError_t conn_launch_pool(const SfConnPool& q, hipStream_t s) {
  SfConnPool p = q;
  if (p.stride <= 1) p.mode = CONN_POOL_NONE;
  p.Po = conn_out_side(p.P, p.mode, p.stride);
  if (p.F < 0 || p.P < 1 || p.Po < 1 || p.C < 8 || p.C % 8) return hipErrorInvalidValue;
  p.C8 = p.C / 8;
  p.scale = (float)p.P / (float)p.Po;
  const int64_t rows = conn_rows(p.F, p.Po, p.nl);
  if (rows <= 0 || rows * p.C > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  if (p.nl != CONN_NL_NONE && !p.newline) return hipErrorInvalidValue;
  p.total = (unsigned)(rows * p.C8);
  const unsigned block = p.total < 65536u ? 64u : 256u;
  unsigned grid = (p.total + block - 1) / block;
  if (grid > 2048u) grid = 2048u;
  const bool planes = p.in_hi != nullptr;
  if (planes && p.out_hi) return sf_launch(sf_connector_pool_kernel<true, 2>, dim3(grid), dim3(block), 0, s, p);
  if (!planes && p.out_f32) return sf_launch(sf_connector_pool_kernel<false, 0>, dim3(grid), dim3(block), 0, s, p);
  if (!planes && p.out_bf16) return sf_launch(sf_connector_pool_kernel<false, 1>, dim3(grid), dim3(block), 0, s, p);
  return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct sf_connector : SfModelHandle {         // weights: image_newline is accepted by every layout and required by those that place it
  sf_connector_config cfg;
  int pool = CONN_POOL_NONE;                  // cfg.pool_mode with stride 1 folded to none
  std::vector<SfDevLinear> lin;
  const float* newline = nullptr;             // [out_dim] or null
};

static std::string conn_linear_key(const sf_connector* c, int i) {
  return c->cfg.depth == 1 ? std::string("mm_projector.") : "mm_projector." + std::to_string(2 * i) + ".";
}

extern "C" int sf_connector_create(const sf_connector_config* cfg, int device, sf_connector** out) {
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: null argument");
  const sf_connector_config& c = *cfg;
  if (c.in_dim <= 0 || c.in_dim % 64) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: in_dim (mm_hidden_size) %d must be a positive multiple of 64 (the GEMM kernels' k-step)", c.in_dim);
  if (c.out_dim <= 0 || c.out_dim % 64) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: out_dim (hidden_size) %d must be a positive multiple of 64", c.out_dim);
  if (c.depth < 0 || c.depth > 16) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: depth %d outside 0..16", c.depth);
  if (c.depth == 0 && c.in_dim != c.out_dim) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: the identity projector needs in_dim == out_dim (%d != %d)", c.in_dim, c.out_dim);
  if (c.pool_mode < 0 || c.pool_mode > 3) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: pool_mode %d (0 none, 1 average, 2 max, 3 bilinear)", c.pool_mode);
  if (c.pool_stride < 1) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: pool_stride %d must be >= 1", c.pool_stride);
  if (c.newline < 0 || c.newline > 3) return sf_set_err(SF_ERR_INVALID, "sf_connector_create: newline %d (0 no_token, 1 one_token, 2 frame, 3 grid)", c.newline);
  sf_connector* h = new sf_connector();
  h->cfg = c;
  h->device = device;
  h->pool = c.pool_stride == 1 ? CONN_POOL_NONE : c.pool_mode;
  SfWeightStore& w = h->weights;
  w.noun = "connector";
  w.prefix = "model.";
  w.dtype_msg = "sf_connector_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
  w.all_required = false;
  for (int i = 0; i < c.depth; ++i) {
    const std::string p = conn_linear_key(h, i);
    w.expect_linear(p, c.out_dim, i ? c.out_dim : c.in_dim);
    w.required.push_back(p + "weight");
    w.required.push_back(p + "bias");
  }
  w.expected["image_newline"] = {c.out_dim};
  if (c.newline != CONN_NL_NONE) w.required.push_back("image_newline");
  *out = h;
  return SF_OK;
}

extern "C" void sf_connector_destroy(sf_connector* c) { delete c; }

extern "C" int sf_connector_load_tensor(sf_connector* c, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  return sf_model_load_tensor(c, "sf_connector_load_tensor", key, host_ptr, dtype, shape, ndim);
}

extern "C" int sf_connector_missing_weights(sf_connector* c) { return sf_model_missing_weights(c); }

// the weights rounded (bf16 mode) or split into hi + lo planes (bf16x3) ONCE, here: no per-call conversion of 3584^2 fp32 values.
// Makes the handle's device current and leaves it so, as the encoder's and the text tower's finalize do (stated in the header).
extern "C" int sf_connector_finalize(sf_connector* c, int compute) {
  SF_TRY(sf_model_begin_finalize(c, compute));
  c->lin.assign(c->cfg.depth, SfDevLinear());
  for (int i = 0; i < c->cfg.depth; ++i) {
    const std::string p = conn_linear_key(c, i);
    SF_TRY(sf_upload_linear(c->dev, c->weights.data(p + "weight"), &c->weights.data(p + "bias"), c->cfg.out_dim, i ? c->cfg.out_dim : c->cfg.in_dim,
                            c->cfg.out_dim, compute == SF_COMPUTE_BF16X3, &c->lin[i]));
  }
  if (c->cfg.newline != CONN_NL_NONE) SF_TRY(c->dev.upload(c->weights.data("image_newline"), &c->newline));
  c->finalized = true;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
struct ConnPlan {
  int Po;                  // output cells per side
  int64_t M, Mp, rows;     // input rows, rows of the last GEMM, rows of the output sequence
  bool pool_first;         // average / bilinear: role (a) in front of the last Linear
};

static int conn_plan(const sf_connector* c, int F, int P, ConnPlan* pl) {
  if (!c) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (F < 1) return sf_set_err(SF_ERR_INVALID, "sf_connector: %d frames", F);
  if (P < 1) return sf_set_err(SF_ERR_INVALID, "sf_connector: %d patches per side", P);
  pl->Po = conn_out_side(P, c->pool, c->cfg.pool_stride);
  if (pl->Po < 1) return sf_set_err(SF_ERR_INVALID, "sf_connector: a %d x %d grid pooled with stride %d leaves no cell", P, P, c->cfg.pool_stride);
  pl->M = (int64_t)F * P * P;
  pl->pool_first = c->cfg.depth >= 1 && (c->pool == CONN_POOL_AVERAGE || c->pool == CONN_POOL_BILINEAR);
  pl->Mp = pl->pool_first ? (int64_t)F * pl->Po * pl->Po : pl->M;
  pl->rows = conn_rows(F, pl->Po, c->cfg.newline);
  const int64_t wide = c->cfg.in_dim > c->cfg.out_dim ? c->cfg.in_dim : c->cfg.out_dim;
  if (pl->M * wide > (int64_t)0x7fffffff || pl->rows * c->cfg.out_dim > (int64_t)0x7fffffff)
    return sf_set_err(SF_ERR_CAPACITY, "sf_connector: %d frames of %d x %d patches exceed 2^31 - 1 elements per activation; project in chunks", F, P, P);
  return SF_OK;
}

struct ConnWorkspace {
  SfPlanes x;                          // the split input [M, in_dim]
  SfPlanes act[2];                     // GELU outputs [M, out_dim], ping-pong from depth 3 up
  SfPlanes pool;                       // role (a) output [Mp, K of the last Linear]
  float* y;                            // the last Linear's output [Mp, out_dim]
  size_t bytes;
};

static ConnWorkspace conn_carve(const sf_connector* c, const ConnPlan& pl, void* base) {
  ConnWorkspace w;
  memset(&w, 0, sizeof(w));
  SfCarver cv(base, c->compute == SF_COMPUTE_BF16X3);
  const size_t M = (size_t)pl.M, Mp = (size_t)pl.Mp, Din = c->cfg.in_dim, Dout = c->cfg.out_dim;
  const int depth = c->cfg.depth;
  if (depth >= 1) {
    w.x = cv.planes(M * Din);
    for (int i = 0; i < (depth >= 3 ? 2 : depth >= 2 ? 1 : 0); ++i) w.act[i] = cv.planes(M * Dout);
    if (pl.pool_first) w.pool = cv.planes(Mp * (depth == 1 ? Din : Dout));
    w.y = cv.take<float>(Mp * Dout);
  }
  w.bytes = cv.bytes();
  if (w.bytes == 0) w.bytes = 256;
  return w;
}

extern "C" int sf_connector_num_tokens(sf_connector* c, int F, int P, int64_t* out) {
  if (!out) return sf_set_err(SF_ERR_INVALID, "null argument");
  ConnPlan pl;
  int rc = conn_plan(c, F, P, &pl);
  if (rc) return rc;
  *out = pl.rows;
  return SF_OK;
}

extern "C" int sf_connector_workspace_bytes(sf_connector* c, int F, int P, size_t* out) {
  if (!out) return sf_set_err(SF_ERR_INVALID, "null argument");
  ConnPlan pl;
  int rc = conn_plan(c, F, P, &pl);
  if (rc) return rc;
  SF_TRY(sf_model_check_finalized(c, "sf_connector", true));
  *out = conn_carve(c, pl, nullptr).bytes;
  return SF_OK;
}

extern "C" int sf_connector_forward(sf_connector* c, const float* feats_dev, int F, int P, void* out_dev, int out_dtype, void* workspace_dev,
                                    size_t workspace_bytes, sf_stream stream) {
  ConnPlan pl;
  int rc = conn_plan(c, F, P, &pl);
  if (rc) return rc;
  SF_TRY(sf_model_check_finalized(c, "sf_connector"));
  if (!feats_dev || !out_dev || !workspace_dev) return sf_set_err(SF_ERR_INVALID, "sf_connector_forward: null buffer");
  if (out_dtype != SF_F32 && out_dtype != SF_BF16) return sf_set_err(SF_ERR_INVALID, "sf_connector_forward: out_dtype %d (SF_F32 or SF_BF16)", out_dtype);
  if (((uintptr_t)feats_dev & 15) || ((uintptr_t)out_dev & 15)) return sf_set_err(SF_ERR_INVALID, "sf_connector_forward: features and output must be 16-byte aligned");
  const ConnWorkspace ws = conn_carve(c, pl, workspace_dev);
  SF_TRY(sf_check_workspace("sf_connector_forward", "sf_connector_workspace_bytes", workspace_dev, workspace_bytes, ws.bytes));
  hipStream_t s = (hipStream_t)stream;
  const sf_connector_config& cfg = c->cfg;
  const SfLinearCaller lin{c->compute == SF_COMPUTE_BF16X3, 0, s};      // act 0: erf GELU (nn.GELU() of the reference builder)
  const int depth = cfg.depth;

  SfConnPool place;                      // role (b): the last launch of every schedule
  memset(&place, 0, sizeof(place));
  place.F = F; place.C = cfg.out_dim; place.nl = cfg.newline; place.newline = c->newline;
  if (out_dtype == SF_F32) place.out_f32 = (float*)out_dev; else place.out_bf16 = (bf16_t*)out_dev;

  if (depth == 0) {                      // identity projector: pool and place the features themselves
    place.in_f32 = feats_dev; place.P = P; place.mode = c->pool; place.stride = cfg.pool_stride;
    HIP_TRY(conn_launch_pool(place, s));
    return SF_OK;
  }
  HIP_TRY(sf_launch_split(feats_dev, ws.x.hi, ws.x.lo, (size_t)pl.M * cfg.in_dim, s));
  SfPlanes a = ws.x;
  for (int i = 0; i + 1 < depth; ++i) {
    HIP_TRY(lin.planes(c->lin[i], a, (int)pl.M, ws.act[i & 1], true));
    a = ws.act[i & 1];
  }
  const SfDevLinear& last = c->lin[depth - 1];
  if (pl.pool_first) {                   // role (a): P^2 -> P'^2 rows per frame in front of the last Linear
    SfConnPool q;
    memset(&q, 0, sizeof(q));
    q.in_hi = a.hi; q.in_lo = a.lo;
    q.out_hi = ws.pool.hi; q.out_lo = ws.pool.lo;
    q.F = F; q.P = P; q.C = last.K; q.mode = c->pool; q.stride = cfg.pool_stride; q.nl = CONN_NL_NONE;
    HIP_TRY(conn_launch_pool(q, s));
    a = ws.pool;
  }
  HIP_TRY(lin.f32(last, a, (int)pl.Mp, ws.y));
  place.in_f32 = ws.y;
  if (pl.pool_first) { place.P = pl.Po; place.mode = CONN_POOL_NONE; place.stride = 1; }      // identity taps: rows are placed only
  else { place.P = P; place.mode = c->pool; place.stride = cfg.pool_stride; }
  HIP_TRY(conn_launch_pool(place, s));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// the kernel alone (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_connector_pool(const float* in_f32_dev, const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, int F, int P, int C,
                                    int pool_mode, int pool_stride, int newline, const float* newline_dev, void* out_dev, int out_dtype,
                                    uint16_t* out_hi_dev, uint16_t* out_lo_dev, sf_stream stream) {
  const bool planes = in_hi_dev != nullptr;
  if (planes == (in_f32_dev != nullptr)) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: pass either the fp32 input or the hi (+ lo) planes");
  if (planes ? (!out_hi_dev || out_dev) : (!out_dev || out_hi_dev || out_lo_dev || in_lo_dev))
    return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: planes in -> planes out (out_hi_dev), fp32 in -> out_dev");
  if (!planes && out_dtype != SF_F32 && out_dtype != SF_BF16) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: out_dtype %d (SF_F32 or SF_BF16)", out_dtype);
  if (F < 0 || (F == 0 && newline != CONN_NL_ONE)) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: %d frames", F);
  if (P < 1) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: %d patches per side", P);
  if (C < 8 || C % 8) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: C = %d must be a positive multiple of 8 (16-byte accesses along C)", C);
  if (pool_mode < 0 || pool_mode > 3 || pool_stride < 1 || newline < 0 || newline > 3)
    return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: pool_mode %d, pool_stride %d, newline %d", pool_mode, pool_stride, newline);
  const int mode = pool_stride == 1 ? CONN_POOL_NONE : pool_mode;
  const int Po = conn_out_side(P, mode, pool_stride);
  if (Po < 1) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: a %d x %d grid pooled with stride %d leaves no cell", P, P, pool_stride);
  if (newline != CONN_NL_NONE && !newline_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: newline %d needs newline_dev", newline);
  if ((int64_t)F * P * P * C > (int64_t)0x7fffffff || conn_rows(F, Po, newline) * C > (int64_t)0x7fffffff)
    return sf_set_err(SF_ERR_CAPACITY, "sf_op_connector_pool: %d frames of %d x %d x %d exceed 2^31 - 1 elements", F, P, P, C);
  if (((uintptr_t)in_f32_dev | (uintptr_t)in_hi_dev | (uintptr_t)in_lo_dev | (uintptr_t)newline_dev | (uintptr_t)out_dev | (uintptr_t)out_hi_dev |
       (uintptr_t)out_lo_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "sf_op_connector_pool: every buffer must be 16-byte aligned");
  SfConnPool p;
  memset(&p, 0, sizeof(p));
  p.in_f32 = in_f32_dev; p.in_hi = in_hi_dev; p.in_lo = in_lo_dev;
  if (planes) { p.out_hi = out_hi_dev; p.out_lo = out_lo_dev; }
  else if (out_dtype == SF_F32) p.out_f32 = (float*)out_dev;
  else p.out_bf16 = (bf16_t*)out_dev;
  p.newline = newline_dev;
  p.F = F; p.P = P; p.C = C; p.mode = mode; p.stride = pool_stride; p.nl = newline;
  HIP_TRY(conn_launch_pool(p, (hipStream_t)stream));
  return SF_OK;
}
