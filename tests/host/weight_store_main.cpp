// Stand-alone check of csrc/sf_weights.h, the host half of every native handle.  Built by tests/test_weight_store_host.py with the
// address and undefined-behaviour sanitizers and run as a child process: exit status 0 = every check held.
#include "sf_weights.h"

#include <algorithm>
#include <cinttypes>
#include <cstdlib>

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static void test_bf16() {
  // ties: 0x....8000 rounds to the even upper half, one ulp on either side rounds to the nearer
  CHECK(sf_host_f2bf(from_bits(0x3f808000u)) == 0x3f80);      // tie, lower neighbour even: down
  CHECK(sf_host_f2bf(from_bits(0x3f818000u)) == 0x3f82);      // tie, lower neighbour odd: up
  CHECK(sf_host_f2bf(from_bits(0x3f807fffu)) == 0x3f80);      // just below the tie
  CHECK(sf_host_f2bf(from_bits(0x3f808001u)) == 0x3f81);      // just above the tie
  CHECK(sf_host_f2bf(from_bits(0x3f817fffu)) == 0x3f81);
  CHECK(sf_host_f2bf(from_bits(0x3f818001u)) == 0x3f82);
  CHECK(sf_host_f2bf(from_bits(0xbf808000u)) == 0xbf80);      // the same on the negative side
  CHECK(sf_host_f2bf(from_bits(0xbf818000u)) == 0xbf82);
  CHECK(sf_host_f2bf(0.0f) == 0x0000);
  CHECK(sf_host_f2bf(-0.0f) == 0x8000);
  CHECK(sf_host_f2bf(INFINITY) == 0x7f80);
  CHECK(sf_host_f2bf(-INFINITY) == 0xff80);
  CHECK(sf_host_f2bf(from_bits(0x7f7fffffu)) == 0x7f80);      // the largest finite fp32 rounds up to inf (nearest even)
  CHECK(std::isnan(sf_host_bf2f(sf_host_f2bf(NAN))));
  CHECK(std::isnan(sf_host_bf2f(sf_host_f2bf(-NAN))));
  // every bf16-representable value survives the round trip: walk 8192 bit patterns across the whole range (NaNs aside)
  int walked = 0;
  for (uint32_t b = 0; b < 0x10000u; b += 8) {
    const float x = sf_host_bf2f((uint16_t)b);
    if (std::isnan(x)) continue;
    ++walked;
    CHECK(bits(sf_host_bf2f(sf_host_f2bf(x))) == bits(x));
  }
  CHECK(walked > 8000);
}

// the second formulation: value = (-1)^s * 2^(e - 15) * (1 + m / 1024), subnormals 2^-14 * m / 1024, in double
static float f16_reference(uint16_t h) {
  const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
  double v;
  if (e == 31) v = m ? (double)NAN : (double)INFINITY;
  else if (e == 0) v = std::ldexp((double)m / 1024.0, -14);
  else v = std::ldexp(1.0 + (double)m / 1024.0, e - 15);
  return (float)(s ? -v : v);
}

static void test_f16() {
  for (uint32_t h = 0; h < 0x10000u; ++h) {
    const float got = sf_host_f16_to_f32((uint16_t)h), want = f16_reference((uint16_t)h);
    if (std::isnan(want)) CHECK(std::isnan(got));
    else CHECK(bits(got) == bits(want));
  }
}

static void test_convert() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)1025}) {
    std::vector<float> f32(n), out(n + 1);
    std::vector<double> f64(n);
    std::vector<uint16_t> bf(n), f16(n);
    for (size_t i = 0; i < n; ++i) {
      bf[i] = (uint16_t)(0x3c00 + 7 * i) ;                    // bf16-representable values, so all four sources hold the same numbers
      f32[i] = sf_host_bf2f(bf[i]);
      f64[i] = (double)f32[i];
      f16[i] = (uint16_t)(0x1000 + 23 * i);
    }
    const float guard = 12345.f;
    struct { int dtype; const void* src; } cases[] = {{SF_F32, f32.data()}, {SF_F64, f64.data()}, {SF_BF16, bf.data()}};
    for (const auto& c : cases) {
      std::fill(out.begin(), out.end(), guard);
      CHECK(sf_convert_to_f32(out.data(), c.src, c.dtype, n, false));
      for (size_t i = 0; i < n; ++i) CHECK(bits(out[i]) == bits(f32[i]));
      CHECK(out[n] == guard);                                  // nothing past n is written
    }
    std::fill(out.begin(), out.end(), guard);
    CHECK(sf_convert_to_f32(out.data(), f16.data(), SF_F16, n, true));
    for (size_t i = 0; i < n; ++i) CHECK(bits(out[i]) == bits(f16_reference(f16[i])));
    CHECK(out[n] == guard);
    CHECK(!sf_convert_to_f32(out.data(), f16.data(), SF_F16, n, false));
    CHECK(!sf_convert_to_f32(out.data(), f32.data(), SF_U8, n, true));
    CHECK(!sf_convert_to_f32(out.data(), f32.data(), 99, n, true));
    CHECK(!sf_convert_to_f32(out.data(), f32.data(), -1, n, true));
  }
}

static void test_split_planes() {
  std::vector<float> w;
  uint32_t seed = 12345u;
  for (int i = 0; i < 4096; ++i) {
    seed = seed * 1664525u + 1013904223u;
    const float mant = 1.0f + (float)(seed >> 8) / 16777216.0f;      // [1, 2)
    w.push_back(std::ldexp((i & 1) ? -mant : mant, (int)(seed & 31) - 16));
  }
  w.push_back(0.f);
  std::vector<uint16_t> hi(w.size()), lo(w.size(), 0xabcd);
  sf_split_planes(w.data(), w.size(), true, hi.data(), lo.data());
  for (size_t i = 0; i < w.size(); ++i) {
    const double sum = (double)sf_host_bf2f(hi[i]) + (double)sf_host_bf2f(lo[i]);
    CHECK(std::fabs(sum - (double)w[i]) <= std::ldexp(std::fabs((double)w[i]), -16));      // two 8-bit roundings
    CHECK(hi[i] == sf_host_f2bf(w[i]));
  }
  std::vector<uint16_t> hi2(w.size()), lo2(w.size(), 0xabcd);
  sf_split_planes(w.data(), w.size(), false, hi2.data(), lo2.data());
  CHECK(hi2 == hi);
  for (uint16_t v : lo2) CHECK(v == 0xabcd);
  sf_split_planes(w.data(), w.size(), false, hi2.data(), nullptr);      // a null lo is never dereferenced
  sf_split_planes(nullptr, 0, true, nullptr, nullptr);
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static void test_store() {
  const float v6[6] = {1, 2, 3, 4, 5, 6};
  const int64_t s23[2] = {2, 3}, s32[2] = {3, 2}, s6[1] = {6}, s123[3] = {1, 2, 3}, s1[1] = {1}, s7[1] = {7};
  std::string err;
  {   // the exact-shape rule of the text tower, the connector and the detector
    SfWeightStore st;
    st.noun = "connector";
    st.prefix = "model.";
    st.dtype_msg = "sf_connector_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
    st.all_required = false;
    st.expected["w"] = {2, 3};
    st.expected["b"] = {3};
    st.expected["image_newline"] = {3};
    st.expected["model.inner"] = {1};
    st.required = {"w", "b"};
    CHECK(st.load("nope", v6, SF_F32, s23, 2, &err) == SF_ERR_UNKNOWN_KEY);
    CHECK(err == "'nope' is not a weight of this connector");
    CHECK(st.load("model.model.w", v6, SF_F32, s23, 2, &err) == SF_ERR_UNKNOWN_KEY);      // stripped once only
    CHECK(err == "'model.model.w' is not a weight of this connector");
    CHECK(st.load("model.model.inner", v6, SF_F32, s1, 1, &err) == SF_OK);                 // ... which leaves "model.inner"
    CHECK(st.host.count("model.inner") == 1);
    CHECK(st.load("w", v6, SF_F32, s32, 2, &err) == SF_ERR_INVALID);
    CHECK(err == "'w': shape mismatch");
    CHECK(st.load("w", v6, SF_F32, s6, 1, &err) == SF_ERR_INVALID);                        // the right count in another rank
    CHECK(st.load("w", v6, SF_F32, s123, 3, &err) == SF_ERR_INVALID);
    CHECK(st.load("w", v6, SF_F16, s23, 2, &err) == SF_ERR_INVALID);
    CHECK(err == "sf_connector_load_tensor: dtype 2 unsupported (fp32, fp64, bf16)");
    CHECK(st.host.count("w") == 0);                                                         // a refused tensor is not staged
    CHECK(st.missing(&err) == 2);
    CHECK(err == "missing 2 weights: w b ");                                                // report order = required order
    CHECK(st.load("model.w", v6, SF_F32, s23, 2, &err) == SF_OK);
    CHECK(st.host.count("w") == 1 && st.data("w").size() == 6 && st.data("w")[5] == 6.f);
    CHECK(st.host["w"].shape == std::vector<int64_t>({2, 3}));
    CHECK(st.missing(&err) == 1);
    CHECK(err == "missing 1 weights: b ");
    const double d6[6] = {6, 5, 4, 3, 2, 1};
    CHECK(st.load("w", d6, SF_F64, s23, 2, &err) == SF_OK);                                 // staging twice overwrites
    CHECK(st.host.size() == 2 && st.data("w")[0] == 6.f && st.data("w")[5] == 1.f);
    CHECK(st.load("b", v6, SF_F32, s6, 1, &err) == SF_ERR_INVALID);
    const int64_t s3[1] = {3};
    CHECK(st.load("b", v6, SF_F32, s3, 1, &err) == SF_OK);
    err = "untouched";
    CHECK(st.missing(&err) == 0);                                                           // image_newline is expected, not required
    CHECK(err == "untouched");
  }
  {   // the encoder's rule: any rank with the right element count; dims compared when the rank matches
    SfWeightStore st;
    st.prefix = "timesformer.";
    st.accept_f16 = true;
    st.exact_shape = false;
    st.expected["pos"] = {1, 2, 3};
    st.expected["gate"] = {};
    st.expected["lin"] = {2, 3};
    CHECK(st.load("timesformer.pos", v6, SF_F32, s23, 2, &err) == SF_OK);                   // [2, 3] for [1, 2, 3]
    CHECK(st.load("pos", v6, SF_F32, s123, 3, &err) == SF_OK);
    CHECK(st.load("pos", v6, SF_F32, s7, 1, &err) == SF_ERR_INVALID);
    CHECK(err == "'pos': shape mismatch (7 elements given, 6 expected)");
    CHECK(st.load("lin", v6, SF_F32, s32, 2, &err) == SF_ERR_INVALID);                      // same rank, same count, other dims
    CHECK(err == "'lin': shape mismatch (6 elements given, 6 expected)");
    CHECK(st.load("lin", v6, SF_F32, s6, 1, &err) == SF_OK);
    CHECK(st.load("gate", v6, SF_F32, nullptr, 0, &err) == SF_OK);                          // a scalar such as temporal_attention_gating
    CHECK(st.data("gate").size() == 1 && st.data("gate")[0] == 1.f);
    CHECK(st.load("gate", v6, SF_F32, s1, 1, &err) == SF_OK);                               // ... or as [1]
    const uint16_t one_f16 = 0x3c00;
    CHECK(st.load("gate", &one_f16, SF_F16, s1, 1, &err) == SF_OK && st.data("gate")[0] == 1.f);
    CHECK(st.load("gate", v6, 99, s1, 1, &err) == SF_ERR_INVALID);
    CHECK(err == "unknown dtype 99");
    CHECK(st.load("other", v6, SF_F32, s1, 1, &err) == SF_ERR_UNKNOWN_KEY);
    CHECK(err == "'other' is not a weight of this model");
    CHECK(st.missing(&err) == 0);
  }
  {   // stage(): the first n values of a longer buffer (the detector's position table)
    SfWeightStore st;
    st.expected["pe"] = {2, 3};
    const int64_t s43[2] = {4, 3};
    const float v12[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    CHECK(st.stage("pe", v12, SF_F32, 6, s43, 2, &err) == SF_OK);
    CHECK(st.data("pe").size() == 6 && st.data("pe")[5] == 5.f);
    CHECK(st.stage("pe", v12, SF_F16, 6, s43, 2, &err) == SF_ERR_INVALID);
  }
  {   // the report stops growing after about 800 characters; the count does not
    SfWeightStore st;
    for (int i = 0; i < 120; ++i) st.expected["encoder.layers." + std::to_string(1000 + i) + ".self_attn.out_proj.weight"] = {1};
    const int n = st.missing(&err);
    CHECK(n == 120);
    CHECK(has(err, "missing 120 weights: encoder.layers.1000.self_attn.out_proj.weight "));
    const size_t head = strlen("missing 120 weights: "), key = strlen("encoder.layers.1000.self_attn.out_proj.weight ");
    CHECK(err.size() >= head + 800 && err.size() < head + 800 + key);
    CHECK(!has(err, "encoder.layers.1119."));
    CHECK(st.load("encoder.layers.1000.self_attn.out_proj.weight", v6, SF_F32, s1, 1, &err) == SF_OK);
    CHECK(st.missing(&err) == 119);
  }
}

static void test_carver() {
  SfCarver count(nullptr);
  CHECK(count.take<float>(3) == nullptr);
  CHECK(count.take<uint16_t>(300) == nullptr);
  CHECK(count.take<char>(0) == nullptr);
  CHECK(count.take<double>(5) == nullptr);
  const size_t bytes = (count.off + 255) & ~(size_t)255;
  CHECK(count.off == 1024 + 40);                    // 12 | 256 + 600 = 856 | 1024 + 0 | 1024 + 40
  void* raw = std::aligned_alloc(256, bytes);
  CHECK(raw != nullptr);
  memset(raw, 0, bytes);
  SfCarver real(raw);
  float* a = real.take<float>(3);
  uint16_t* b = real.take<uint16_t>(300);
  char* c = real.take<char>(0);
  double* d = real.take<double>(5);
  CHECK(real.off == count.off);                     // counting and assigning agree
  for (const void* p : {(const void*)a, (const void*)b, (const void*)c, (const void*)d}) CHECK(((uintptr_t)p & 255) == 0);
  CHECK((char*)a == (char*)raw && (char*)b == (char*)raw + 256 && (char*)c == (char*)raw + 1024 && (char*)d == (char*)raw + 1024);
  for (int i = 0; i < 3; ++i) a[i] = 1.f;           // every piece is writable inside the counted size
  for (int i = 0; i < 300; ++i) b[i] = 2;
  for (int i = 0; i < 5; ++i) d[i] = 3.0;
  CHECK((char*)(d + 5) <= (char*)raw + bytes);
  std::free(raw);
}

// expect_linear / expect_affine against the pairs the handles wrote by hand
static void test_expect() {
  SfWeightStore got, want;
  got.expect_linear("layers.0.linear1.", 128, 64);
  want.expected["layers.0.linear1.weight"] = {128, 64};
  want.expected["layers.0.linear1.bias"] = {128};
  got.expect_linear("adapter_1.", 64, 192, false);
  want.expected["adapter_1.weight"] = {64, 192};
  got.expect_affine("layers.0.norm1.", 64);
  want.expected["layers.0.norm1.weight"] = {64};
  want.expected["layers.0.norm1.bias"] = {64};
  got.expect_linear("", 3, 5);                           // the connector's depth-1 prefix ends in the dot itself; an empty one is legal too
  want.expected["weight"] = {3, 5};
  want.expected["bias"] = {3};
  CHECK(got.expected == want.expected);
  CHECK(got.expected.size() == 7 && got.expected.count("adapter_1.bias") == 0);
  CHECK(got.required.empty() && got.host.empty());      // nothing but the table is touched
}

// the plane carve against the two takes it replaces, under both reservation rules, in both modes, counting and assigning
static void test_planes() {
  alignas(256) static char buf[8192];
  const size_t n = 300, m = 77;                          // 600 and 154 bytes: neither a multiple of the 256-byte step
  for (int reserve = 0; reserve < 2; ++reserve)
    for (int split = 0; split < 2; ++split)
      for (char* base : {(char*)nullptr, buf}) {
        SfCarver old(base), cv(base, split != 0, reserve != 0);
        float* f_old = old.take<float>(5);
        uint16_t* hi_old = old.take<uint16_t>(n);
        uint16_t* lo_old = (split || reserve) ? old.take<uint16_t>(n) : nullptr;
        float* g_old = old.take<float>(3);
        float* f = cv.take<float>(5);
        const SfPlanes p = cv.planes(n);
        float* g = cv.take<float>(3);
        CHECK(f == f_old && p.hi == hi_old && g == g_old);
        CHECK(p.lo == (split ? lo_old : nullptr));        // reserved bytes are not handed out in bf16 mode
        CHECK(cv.off == old.off && cv.bytes() == old.bytes());
        CHECK((p.hi == nullptr) == (base == nullptr));    // a sizing pass hands out nothing
        if (!base) CHECK(p.lo == nullptr);
        // several hi planes first, their lo planes after them
        uint16_t* a_old = old.take<uint16_t>(n);
        uint16_t* b_old = old.take<uint16_t>(m);
        uint16_t* al_old = nullptr; uint16_t* bl_old = nullptr;
        if (split || reserve) { al_old = old.take<uint16_t>(n); bl_old = old.take<uint16_t>(m); }
        SfPlanes a, b;
        a.hi = cv.take<uint16_t>(n); b.hi = cv.take<uint16_t>(m);
        a.lo = cv.lo(n); b.lo = cv.lo(m);
        CHECK(a.hi == a_old && b.hi == b_old);
        CHECK(a.lo == (split ? al_old : nullptr) && b.lo == (split ? bl_old : nullptr));
        CHECK(cv.bytes() == old.bytes() && cv.bytes() <= sizeof(buf));
        if (base && split) { a.lo[n - 1] = 1; b.lo[m - 1] = 2; p.lo[n - 1] = 3; }      // inside the buffer (the sanitizer watches)
        // at(): both planes move, null stays null
        const SfPlanes q = p.at(17);
        CHECK(q.hi == (p.hi ? p.hi + 17 : nullptr));
        CHECK(q.lo == (p.lo ? p.lo + 17 : nullptr));
        CHECK(p.at(0).hi == p.hi && p.at(0).lo == p.lo);
      }
  const SfPlanes none;
  CHECK(none.hi == nullptr && none.lo == nullptr && none.at(1000).hi == nullptr && none.at(1000).lo == nullptr);
}

int main() {
  test_expect();
  test_planes();
  test_bf16();
  test_f16();
  test_convert();
  test_split_planes();
  test_store();
  test_carver();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("weight store: all checks passed\n");
  return 0;
}
