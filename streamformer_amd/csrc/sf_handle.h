// Device side of a native model's handle, shared by sf_encoder, sf_text, sf_connector, sf_oad, sf_pixdec and sf_maskdec: the device
// allocations a finalize owns, a Linear's bf16 planes and a LayerNorm's affine pair with their uploads, the GEMM arguments every Linear
// starts from and SfLinearCaller, the three calls most Linears are, and SfModelHandle, the part of a tail model's handle (everything but
// the encoder's) and of its entry points that does not depend on the model.  The host half, SfPlanes and the carver included, is
// sf_weights.h.
#pragma once
#include "sf_common.h"
#include "sf_internal.h"
#include "sf_weights.h"

#include <algorithm>
#include <type_traits>

#define SF_TRY(x)             \
  do {                        \
    const int rc_ = (x);      \
    if (rc_) return rc_;      \
  } while (0)

static inline int sf_check_compute_mode(int compute) {
  if (compute != SF_COMPUTE_BF16 && compute != SF_COMPUTE_BF16X3) return sf_set_err(SF_ERR_INVALID, "unknown compute mode %d", compute);
  return SF_OK;
}

struct SfDevLinear {          // y = x W^T + b ; W [N, K] as bf16 planes (w_lo: the accurate mode's second plane, else null)
  const bf16_t* w_hi = nullptr;
  const bf16_t* w_lo = nullptr;
  const float* bias = nullptr;
  int N = 0, K = 0;
};
struct SfDevLN { const float* g = nullptr; const float* b = nullptr; };

// what a finalize put on the device; freed together by the next finalize and by destroy
struct SfDeviceAllocs {
  std::vector<void*> ptrs;
  size_t uploaded = 0;        // bytes copied by upload() since the last free_all()

  int alloc(size_t bytes, void** out) {
    HIP_TRY(hipMalloc(out, bytes));
    ptrs.push_back(*out);
    return SF_OK;
  }
  template <typename T, typename P>      // P: T or const T
  int upload(const std::vector<T>& h, P** out) {
    static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "upload: pointer type");
    void* p = nullptr;
    const size_t bytes = h.size() * sizeof(T);
    SF_TRY(alloc(bytes ? bytes : 16, &p));
    if (bytes) HIP_TRY(hipMemcpy(p, h.data(), bytes, hipMemcpyHostToDevice));
    uploaded += bytes;
    *out = (P*)p;
    return SF_OK;
  }
  void free_all() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
    uploaded = 0;
  }
};

// ------------------------------------------------------------------------------------------------
// What sf_text, sf_connector, sf_oad, sf_pixdec and sf_maskdec share: a handle derives from SfModelHandle and brings its config
// validation, its expected-key table, its uploads, its plan, carve and launch sequence.  `family` below is the prefix of its entry points ("sf_text").
// ------------------------------------------------------------------------------------------------
struct SfModelHandle {
  int device = 0;
  SfWeightStore weights;
  bool finalized = false;       // set at the end of *_finalize, cleared by every staged tensor
  int compute = SF_COMPUTE_BF16;
  SfDeviceAllocs dev;
  ~SfModelHandle() { dev.free_all(); }
};

// *_load_tensor in two steps, for a family that stages some key by a rule of its own between them
static inline int sf_model_load_args(const SfModelHandle* h, const char* who, const char* key, const void* host_ptr, const int64_t* shape, int ndim) {
  if (!h || !key || !host_ptr || ndim < 0 || (ndim && !shape)) return sf_set_err(SF_ERR_INVALID, "%s: null argument", who);
  return SF_OK;
}
static inline int sf_model_staged(SfModelHandle* h, int rc, const std::string& err) {      // rc, err: what weights.load / stage gave
  if (rc) return sf_set_err(rc, "%s", err.c_str());
  h->finalized = false;
  return SF_OK;
}
static inline int sf_model_load_tensor(SfModelHandle* h, const char* who, const char* key, const void* host_ptr, int dtype, const int64_t* shape,
                                       int ndim) {
  SF_TRY(sf_model_load_args(h, who, key, host_ptr, shape, ndim));
  std::string err;
  const int rc = h->weights.load(key, host_ptr, dtype, shape, ndim, &err);
  return sf_model_staged(h, rc, err);
}

static inline int sf_model_missing_weights(SfModelHandle* h) {
  if (!h) return sf_set_err(SF_ERR_INVALID, "null handle");
  std::string err;
  const int missing = h->weights.missing(&err);
  if (missing) sf_set_err(SF_ERR_STATE, "%s", err.c_str());
  return missing;
}

// The opening of every *_finalize: refuses a null handle, an unknown mode and missing weights, makes the handle's device current and
// leaves it so, frees what the last finalize put on the device and records the mode.  The handle counts as not finalized until the
// caller sets h->finalized after its last upload, so a finalize that fails half-way leaves no freed pointer in use.
static inline int sf_model_begin_finalize(SfModelHandle* h, int compute) {
  if (!h) return sf_set_err(SF_ERR_INVALID, "null handle");
  SF_TRY(sf_check_compute_mode(compute));
  if (sf_model_missing_weights(h)) return SF_ERR_STATE;
  HIP_TRY(hipSetDevice(h->device));
  h->dev.free_all();
  h->finalized = false;
  h->compute = compute;
  return SF_OK;
}

// The refusals of a forward entry.  sizing: the wording of the *_workspace_bytes entry points.
static inline int sf_model_check_finalized(const SfModelHandle* h, const char* family, bool sizing = false) {
  if (h->finalized) return SF_OK;
  return sf_set_err(SF_ERR_STATE, sizing ? "%s_finalize has not run (the workspace depends on the compute mode)" : "%s_finalize has not run (or weights were loaded after it)", family);
}
// who: the entry point; sizer: the function that tells `need`
static inline int sf_check_workspace(const char* who, const char* sizer, const void* workspace, size_t given, size_t need) {
  if ((uintptr_t)workspace & 255) return sf_set_err(SF_ERR_INVALID, "%s: workspace must be 256-byte aligned", who);
  if (given < need) return sf_set_err(SF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (%s)", who, given, need, sizer);
  return SF_OK;
}

// [N, K] weight (+ bias) -> bf16 hi (+ lo) planes on the device, uploaded in the order hi, lo, bias.  Np >= N zero-pads rows and bias
// (out->N = Np); without want_lo, out->w_lo is null.  The rounding happens ONCE, here: no per-call conversion of the weights.
static inline int sf_upload_linear(SfDeviceAllocs& dev, const std::vector<float>& w, const std::vector<float>* bias, int N, int K, int Np,
                                   bool want_lo, SfDevLinear* out) {
  const size_t np = (size_t)Np * K;
  std::vector<uint16_t> hi(np, 0), lo(want_lo ? np : 0, 0);
  sf_split_planes(w.data(), (size_t)N * K, want_lo, hi.data(), lo.data());
  SF_TRY(dev.upload(hi, &out->w_hi));
  out->w_lo = nullptr;
  if (want_lo) SF_TRY(dev.upload(lo, &out->w_lo));
  if (bias && Np == N) SF_TRY(dev.upload(*bias, &out->bias));
  else if (bias) {
    std::vector<float> b((size_t)Np, 0.f);
    std::copy(bias->begin(), bias->end(), b.begin());
    SF_TRY(dev.upload(b, &out->bias));
  }
  out->N = Np;
  out->K = K;
  return SF_OK;
}

static inline int sf_upload_ln(SfDeviceAllocs& dev, SfWeightStore& w, const std::string& prefix, SfDevLN* out) {      // weight, then bias
  SF_TRY(dev.upload(w.data(prefix + "weight"), &out->g));
  return dev.upload(w.data(prefix + "bias"), &out->b);
}

// rows [row0, row0 + rows) of an uploaded Linear as a Linear of their own (a packed in_proj's q, k | v, ...), with the bias given
static inline SfDevLinear sf_linear_rows(const SfDevLinear& lin, int row0, int rows, const float* bias) {
  SfDevLinear o = lin;
  o.w_hi = lin.w_hi + (size_t)row0 * lin.K;
  o.w_lo = lin.w_lo ? lin.w_lo + (size_t)row0 * lin.K : nullptr;
  o.bias = bias;
  o.N = rows;
  return o;
}

// The fields every Linear's GEMM shares; a call site then sets what is special about it (outputs, residual, LayerNorm fold, row
// remap) by field name and launches with the same `split`.
static inline SfGemmArgs sf_linear_args(const SfDevLinear& lin, const bf16_t* a_hi, const bf16_t* a_lo, int M, int epi, int act, bool split) {
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = a_hi; g.a_lo = split ? a_lo : nullptr;
  g.w_hi = lin.w_hi; g.w_lo = split ? lin.w_lo : nullptr;
  g.bias = lin.bias;
  g.M = M; g.N = lin.N; g.K = lin.K; g.ldc = lin.N;
  g.epi = epi; g.act = act; g.alpha = 1.f;
  return g;
}

// A model's forward says its compute mode, its activation (0 erf GELU, 1 tanh GELU, 2 ReLU: read by the activated epilogue only) and
// its stream once, and then runs a Linear on `rows` rows of the planes `a` in one of three ways.  A GEMM that needs a field these do
// not set starts from sf_linear_args itself.
struct SfLinearCaller {
  bool split;
  int act;
  hipStream_t stream;

  hipError_t f32(const SfDevLinear& lin, const SfPlanes& a, int rows, float* out, int ldc = 0) const {      // ldc 0: lin.N, dense rows
    SfGemmArgs g = sf_linear_args(lin, a.hi, a.lo, rows, SF_EPI_F32, act, split);
    g.out_f32 = out;
    if (ldc) g.ldc = ldc;
    return sf_launch_gemm(g, split, stream);
  }
  hipError_t planes(const SfDevLinear& lin, const SfPlanes& a, int rows, const SfPlanes& out, bool activated) const {
    SfGemmArgs g = sf_linear_args(lin, a.hi, a.lo, rows, activated ? SF_EPI_ACT_BF16 : SF_EPI_BF16, act, split);
    g.out_hi = out.hi; g.out_lo = out.lo;
    return sf_launch_gemm(g, split, stream);
  }
  hipError_t resid(const SfDevLinear& lin, const SfPlanes& a, int rows, const float* resid, float* out) const {      // out = resid + a W^T + b
    SfGemmArgs g = sf_linear_args(lin, a.hi, a.lo, rows, SF_EPI_RESID_F32, act, split);
    g.resid = resid; g.out_f32 = out;
    return sf_launch_gemm(g, split, stream);
  }
};
