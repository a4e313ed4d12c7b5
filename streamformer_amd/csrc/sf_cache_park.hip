// Parking a stream of the temporal KV-cache: one launch gathers the K and V columns of the frames a stream holds, over all layers,
// into one contiguous blob (export); one launch scatters such a blob into a slab (import).
//
// A slab of a layer's cache is [cap, N, 3D] rows of [q | k | v]; a stream that holds `held` frames owns its first held * N rows
// (slot = frame mod cap, so a ring that has wrapped owns all of them).  The q third of a cached row is dead once its frame has been
// attended — only new frames query — so the blob carries the k | v two thirds: [L][held * N][2D] elements of the cache's own type.
// Blob row j of a layer IS slab row j: ring slots keep their places, nothing is linearised.
//
// Pure copy: 16-byte vectors, four independent loads in flight per thread before the first store, grid capped near 8 workgroups
// per CU and grid-strided.  Every index is below args.nvec = held * N * vpr, the rows the stream owns.
#include "sf_common.h"

template <bool EXPORT>
__global__ __launch_bounds__(256) void sf_cache_park_kernel(const SfParkArgs a) {
  const int l = blockIdx.y;
  char* slab = a.layer[l] + a.slab_off + a.kv_off;                 // k column of the stream's row 0 in this layer
  char* blob = a.blob + (size_t)(a.layer0 + l) * a.layer_blob_bytes;
  const uint32_t step = gridDim.x * 256u;
  for (uint32_t v0 = blockIdx.x * 256u + threadIdx.x; v0 < a.nvec; v0 += 4u * step) {
    u32x4_t r[4];
    size_t so[4], bo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t v = v0 + (uint32_t)k * step;
      const uint32_t row = v / a.vpr, c = v - row * a.vpr;
      so[k] = (size_t)row * a.row_bytes + (size_t)c * 16;
      bo[k] = (size_t)v * 16;
      // v0 + k * step cannot wrap: the launch keeps nvec + 4 * step below 2^32
      if (v < a.nvec) r[k] = *reinterpret_cast<const u32x4_t*>(EXPORT ? slab + so[k] : blob + bo[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v0 + (uint32_t)k * step < a.nvec) *reinterpret_cast<u32x4_t*>(EXPORT ? blob + bo[k] : slab + so[k]) = r[k];
  }
}

hipError_t sf_launch_cache_park(const SfParkArgs& a, int layers, bool do_export, hipStream_t s) {
  if (layers <= 0 || layers > SF_PARK_MAX_LAYERS || !a.blob || !a.vpr || a.nvec > 0x7fffffffu) return hipErrorInvalidValue;
  if ((a.row_bytes | a.kv_off | a.slab_off | a.layer_blob_bytes | (size_t)a.blob) & 15) return hipErrorInvalidValue;
  if ((size_t)a.nvec * 16 != a.layer_blob_bytes) return hipErrorInvalidValue;
  for (int l = 0; l < layers; ++l)
    if (!a.layer[l] || ((size_t)a.layer[l] & 15)) return hipErrorInvalidValue;
  if (!a.nvec) return hipSuccess;
  // ~2048 workgroups over the layers (8 per CU), 1024 vectors = 16 KiB per workgroup and sweep
  unsigned per_layer = (2048 + layers - 1) / layers, need = (a.nvec + 1023u) / 1024u;
  const dim3 grid(need < per_layer ? need : per_layer, layers);
  if (do_export) return sf_launch(sf_cache_park_kernel<true>, grid, dim3(256), 0, s, a);
  return sf_launch(sf_cache_park_kernel<false>, grid, dim3(256), 0, s, a);
}
