// Host side of a native model's handle: staging of named weights and their expected-key table, bf16 rounding, workspace carving and
// the bf16 plane pair the carver hands out.  Plain C++17 with nothing from HIP: every handle built on SfWeightStore (sf_encoder, sf_text,
// sf_connector, sf_oad, sf_pixdec, sf_maskdec) shares it, and tests/host/weight_store_main.cpp checks it on a CPU under sanitizers.  The
// device half (uploads, GEMM arguments and calls) is sf_handle.h.
#pragma once
#include "../../include/streamformer_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------
// number formats
// ------------------------------------------------------------------------------------------------
// round to nearest even; a NaN stays a NaN (the payloads a caller can produce keep a mantissa bit in the upper half)
inline uint16_t sf_host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float sf_host_bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline float sf_host_f16_to_f32(uint16_t h) {
  const uint32_t s = (h >> 15) & 1, ex = (h >> 10) & 31, m = h & 1023;
  float v;
  if (ex == 0) v = ldexpf((float)m, -24);
  else if (ex == 31) v = m ? NAN : INFINITY;
  else v = ldexpf((float)(m | 1024), (int)ex - 25);
  return s ? -v : v;
}

// n values of an sf_dtype -> fp32.  false: a dtype no handle stages (or SF_F16 where the handle's contract leaves it out)
inline bool sf_convert_to_f32(float* dst, const void* src, int dtype, size_t n, bool accept_f16) {
  switch (dtype) {
    case SF_F32: if (n) memcpy(dst, src, n * 4); return true;
    case SF_F64: for (size_t i = 0; i < n; ++i) dst[i] = (float)((const double*)src)[i]; return true;
    case SF_BF16: for (size_t i = 0; i < n; ++i) dst[i] = sf_host_bf2f(((const uint16_t*)src)[i]); return true;
    case SF_F16:
      if (!accept_f16) return false;
      for (size_t i = 0; i < n; ++i) dst[i] = sf_host_f16_to_f32(((const uint16_t*)src)[i]);
      return true;
    default: return false;
  }
}

// w -> the bf16 plane hi = bf16(w) and, with want_lo, lo = bf16(w - hi): what the GEMMs read in the two compute modes.
// Without want_lo, lo is not touched (it may be null).
inline void sf_split_planes(const float* w, size_t n, bool want_lo, uint16_t* hi, uint16_t* lo) {
  for (size_t i = 0; i < n; ++i) {
    hi[i] = sf_host_f2bf(w[i]);
    if (want_lo) lo[i] = sf_host_f2bf(w[i] - sf_host_bf2f(hi[i]));
  }
}

// ------------------------------------------------------------------------------------------------
// staged weights
// ------------------------------------------------------------------------------------------------
struct SfHostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// The weights of one handle between *_load_tensor and *_finalize: which keys it takes, with which shapes, and the fp32 copies staged
// so far.  Every call returns an sf_status; on failure *err holds the message for sf_last_error().
struct SfWeightStore {
  std::map<std::string, std::vector<int64_t>> expected;      // every key load() accepts
  std::vector<std::string> required;                         // with all_required == false: the keys finalize needs, in report order
  bool all_required = true;
  std::map<std::string, SfHostTensor> host;                  // staged fp32 copies
  // per handle, set once at creation
  const char* noun = "model";            // "'%s' is not a weight of this <noun>"
  const char* prefix = "";               // a checkpoint wrapper's leading "<name>." is stripped (once) from incoming keys
  const char* dtype_msg = "unknown dtype %d";
  bool accept_f16 = false;
  bool exact_shape = true;               // false: any ndim with the right element count; dims compared only when ndim matches

  static int fail(std::string* err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *err = buf;
    return code;
  }

  // the expected shape of `key` (null: not a weight of this handle); *k is the key as the store files it
  const std::vector<int64_t>* lookup(const char* key, std::string* k) const {
    *k = key;
    const size_t pl = strlen(prefix);
    if (pl && k->compare(0, pl, prefix) == 0) k->erase(0, pl);
    auto it = expected.find(*k);
    return it == expected.end() ? nullptr : &it->second;
  }

  // the handle's shape rule; *n and *ne are the element counts given and expected
  bool shape_ok(const std::vector<int64_t>& want, const int64_t* shape, int ndim, size_t* n, size_t* ne) const {
    *n = 1; *ne = 1;
    for (int i = 0; i < ndim; ++i) *n *= (size_t)shape[i];
    for (int64_t d : want) *ne *= (size_t)d;
    const bool same_rank = (int)want.size() == ndim;
    bool same = exact_shape ? same_rank : *n == *ne;
    if (same && same_rank)
      for (int i = 0; i < ndim; ++i) same = same && want[i] == shape[i];
    return same;
  }

  // the first n values at src, converted, become the staged tensor k (an earlier one is replaced)
  int stage(const std::string& k, const void* src, int dtype, size_t n, const int64_t* shape, int ndim, std::string* err) {
    SfHostTensor t;
    t.shape.assign(shape, shape + ndim);
    t.data.resize(n);
    if (!sf_convert_to_f32(t.data.data(), src, dtype, n, accept_f16)) return fail(err, SF_ERR_INVALID, dtype_msg, dtype);
    host[k] = std::move(t);
    return SF_OK;
  }

  int load(const char* key, const void* src, int dtype, const int64_t* shape, int ndim, std::string* err) {
    std::string k;
    const std::vector<int64_t>* want = lookup(key, &k);
    if (!want) return fail(err, SF_ERR_UNKNOWN_KEY, "'%s' is not a weight of this %s", key, noun);
    size_t n, ne;
    if (!shape_ok(*want, shape, ndim, &n, &ne))
      return exact_shape ? fail(err, SF_ERR_INVALID, "'%s': shape mismatch", key)
                         : fail(err, SF_ERR_INVALID, "'%s': shape mismatch (%zu elements given, %zu expected)", key, n, ne);
    return stage(k, src, dtype, n, shape, ndim, err);
  }

  // how many required keys are not staged; *err names them (up to about 800 characters)
  int missing(std::string* err) const {
    int count = 0;
    std::string names;
    auto want = [&](const std::string& k) {
      if (host.count(k)) return;
      ++count;
      if (names.size() < 800) names += k + " ";
    };
    if (all_required) for (const auto& kv : expected) want(kv.first);
    else for (const std::string& k : required) want(k);
    if (count) fail(err, SF_ERR_STATE, "missing %d weights: %s", count, names.c_str());
    return count;
  }

  std::vector<float>& data(const std::string& k) { return host[k].data; }

  // the keys of an nn.Linear [N, K] under `p` ("....linear1."), and of a LayerNorm / GroupNorm affine pair over C channels
  void expect_linear(const std::string& p, int64_t N, int64_t K, bool bias = true) {
    expected[p + "weight"] = {N, K};
    if (bias) expected[p + "bias"] = {N};
  }
  void expect_affine(const std::string& p, int64_t C) {
    expected[p + "weight"] = {C};
    expected[p + "bias"] = {C};
  }
};

// ------------------------------------------------------------------------------------------------
// workspace carving: 256-byte aligned pieces of one buffer.  A null base only counts (the *_workspace_bytes entry points).
// ------------------------------------------------------------------------------------------------
// An activation as the GEMMs read it: the bf16 plane hi and, in bf16x3 mode only, the plane lo of what hi rounded away.  lo is null in
// bf16 mode, so a launch passes p.hi, p.lo as they are and a kernel that is handed a lo plane writes it.
struct SfPlanes {
  uint16_t* hi = nullptr;
  uint16_t* lo = nullptr;
  SfPlanes at(size_t elements) const {      // the same pair `elements` further on; null stays null (lo in bf16 mode, both while sizing)
    SfPlanes p;
    p.hi = hi ? hi + elements : nullptr;
    p.lo = lo ? lo + elements : nullptr;
    return p;
  }
};

struct SfCarver {
  char* base;
  size_t off = 0;
  bool split = false;           // bf16x3 mode: lo planes are handed out
  bool reserve_lo = false;      // a lo plane's bytes are set aside in bf16 mode too (a workspace whose size does not depend on the mode)
  explicit SfCarver(void* b, bool split_ = false, bool reserve_lo_ = false) : base((char*)b), split(split_), reserve_lo(reserve_lo_) {}
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  // the lo plane of n elements: where a model takes several hi planes first and their lo planes after them
  uint16_t* lo(size_t n) {
    uint16_t* p = split || reserve_lo ? take<uint16_t>(n) : nullptr;
    return split ? p : nullptr;
  }
  SfPlanes planes(size_t n) {      // hi, then lo
    SfPlanes p;
    p.hi = take<uint16_t>(n);
    p.lo = lo(n);
    return p;
  }
  size_t bytes() const { return (off + 255) & ~(size_t)255; }      // what a workspace holding every piece taken so far needs
};
