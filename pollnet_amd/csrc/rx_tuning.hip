// Tuning library (libpollnet_amd_tuning.so, include/pollnet_amd_tuning.h), RX side: the same-run
// bandwidth ceilings bench.py reports beside the production kernel, the match-streams variants and
// the spin / doorbell helpers.  Never linked into or loaded by the product path.  The classify
// kernel's own A/B variants are retired ("Retired RX variants").
#include "rx_classify.hpp"
#include "stream_match.hpp"

namespace {
using pn_internal::g_err;
using pn_internal::hip_err;
using pn_internal::set_err;

__global__ __launch_bounds__(256) void calib_stream_read_kernel(const u32x4* src, uint64_t n16, uint32_t* sink) {
  // the whole grid sweeps the buffer front to back, one 16-B coalesced load per lane per step
  uint32_t acc = 0;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256) {
    const u32x4 v = src[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9E3779B9u) sink[blockIdx.x] = acc; // keeps the loads live; practically never stores
}

// Test helper: one lane holds its stream until the host stores non-zero to *go (pinned host
// memory) or max_ticks of the device wall clock pass (always exits), then stores 1 (released)
// or 2 (timed out) to *done.  Stands for unrelated work in flight on a foreign stream.
__global__ __launch_bounds__(64) void spin_wait_kernel(const uint32_t* go, uint32_t* done, uint64_t max_ticks) {
  if (threadIdx.x != 0) return;
  const uint64_t t0 = wall_clock64();
  uint32_t r = 2;
  while (wall_clock64() - t0 < max_ticks) {
    if (__hip_atomic_load(go, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
      r = 1;
      break;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  __hip_atomic_store(done, r, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Latency probe (round 5, bench/bench_doorbell): how fast can a resident kernel answer the host?  One lane
// watches *bell (pinned host memory) and copies every new value to *echo; it ends at the value 0xFFFFFFFF or
// after max_idle_ticks of the device wall clock without a new value (always exits).  once = 1: answer the
// value already there and end (the launch-per-request form the product uses today).
__global__ __launch_bounds__(64) void doorbell_echo_kernel(const uint32_t* bell, uint32_t* echo, uint64_t max_idle_ticks,
                                                            uint32_t once, uint32_t sleep) {
  if (threadIdx.x != 0) return;
  uint32_t last = 0;
  uint64_t t_last = wall_clock64();
  for (;;) {
    // relaxed in the loop (a system-scope load reads memory; an acquire would invalidate the caches every
    // iteration); the acquire fence once a new value has arrived
    const uint32_t v = __hip_atomic_load(bell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (v == 0xFFFFFFFFu) break;
    if (v != last || once) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      last = v;
      __hip_atomic_store(echo, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      if (once) break;
      t_last = wall_clock64();
    } else if (wall_clock64() - t_last > max_idle_ticks) {
      break;
    }
    if (sleep) __builtin_amdgcn_s_sleep(1);
  }
}

// The doorbell answered from a pipelined poll: K relaxed system-scope reads of the bell's 64-B line in flight (lane
// i reads word i & 15: the service mailbox's shape, no branch around the load), issued `gap` x 64 clocks apart; each is checked when it returns (the
// value stays in a VGPR until its readlane, so the compiler waits for the oldest read only: vmcnt(K - 1)).  A new
// value is seen about one gap after it lands rather than up to one read round trip later.  Reads issued before a value
// arrived return older values: only a larger value counts.
template <int K>
__global__ __launch_bounds__(64) void doorbell_echo_pipe_kernel(const uint32_t* bell, uint32_t* echo,
                                                                uint64_t max_idle_ticks, uint32_t gap) {
  const int lane = threadIdx.x;
  uint32_t last = 0;
  uint64_t t_last = wall_clock64();
  uint32_t q[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    q[j] = __hip_atomic_load(bell + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (uint32_t g = 0; g < gap; ++g) __builtin_amdgcn_s_sleep(1);
  }
  // no return inside the loop: an exit path there makes the compiler drain every read at the loop head (vmcnt(0))
  bool go = true;
  while (go) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t v = (uint32_t)__builtin_amdgcn_readlane(q[j], 0);
      if (v == 0xFFFFFFFFu) {
        go = false;
      } else if ((int32_t)(v - last) > 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        last = v;
        if (lane == 0) __hip_atomic_store(echo, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        t_last = wall_clock64();
      } else if (wall_clock64() - t_last > max_idle_ticks) {
        go = false;
      }
      q[j] = __hip_atomic_load(bell + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      for (uint32_t g = 0; g < gap; ++g) __builtin_amdgcn_s_sleep(1);
    }
  }
}

// Read-only ceilings for the slot layout (no header work, no arithmetic): each wave
// streams the first `bytes` of each of its 64 slots with the RX kernel's 1-KiB
// buffer loads, 8 slots per batch.  STORE = 16 / 8: plus a per-slot record store
// of that many bytes at the wave's end (sink holds n x 16 B), the RX kernel's
// write pattern.
template <int STORE>
__global__ __launch_bounds__(kWave) void calib_slot_read_kernel(const uint8_t* base, uint32_t n, uint32_t stride,
                                                               uint32_t bytes, uint32_t* sink) {
  const int lane = threadIdx.x;
  const uint32_t wave_base = blockIdx.x * kFramesPerWave;
  if (wave_base >= n) return;
  const uint32_t n_here = min((uint32_t)kFramesPerWave, n - wave_base);
  const uint8_t* wb = base + (uint64_t)wave_base * stride;
  uint32_t acc = 0;
  for (uint32_t b0 = 0; b0 < n_here; b0 += kBatch) {
    u32x4 w0s[kBatch], w1s[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const uint32_t nb = (b0 + j < n_here) ? bytes : 0u;
      const __amdgpu_buffer_rsrc_t rs = frame_rsrc(wb + (uint64_t)(b0 + j) * stride, nb);
      w0s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, 0, 0);
      w1s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, 1024 + lane * 16, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kBatch; ++j) acc ^= w0s[j].x ^ w0s[j].y ^ w0s[j].z ^ w0s[j].w ^ w1s[j].x ^ w1s[j].y ^ w1s[j].z ^ w1s[j].w;
  }
  if constexpr (STORE == 16) {
    if (lane < (int)n_here) {
      u32x4 r = {acc, acc ^ 1u, acc ^ 2u, acc ^ 3u};
      *reinterpret_cast<u32x4*>(sink + 4 * (uint64_t)(wave_base + lane)) = r;
    }
  } else if constexpr (STORE == 8) {
    if (lane < (int)n_here) *reinterpret_cast<uint64_t*>(sink + 2 * (uint64_t)(wave_base + lane)) = ((uint64_t)acc << 32) | acc;
  } else {
    if (acc == 0x9E3779B9u) sink[blockIdx.x] = acc;
  }
}

// Ceiling for variable-length frames (C3/C5 slot rings): slot i's first lens[i] bytes (the
// frame's lines, from the slot start to the frame's pad byte), read with the RX kernel's load
// pattern, workgroup order (each XCD a contiguous eighth) and LDS occupancy cap, no arithmetic;
// STORE = 16 adds the 16-B records.  Out-of-range dwords of a line cost no extra traffic.
template <int STORE>
__global__ __launch_bounds__(kWave) void calib_slot_read_var_kernel(const uint8_t* base, uint32_t n, uint32_t stride,
                                                                   const uint32_t* lens, uint32_t* sink) {
  __shared__ uint32_t pad_lds[512];
  const int lane = threadIdx.x;
  pad_lds[lane] = lane;
  // never true: keeps the padding allocated (wave-uniform, so n and the descriptors stay scalar)
  if (__builtin_amdgcn_readfirstlane(pad_lds[(lane + 1) & 63]) == 0x7fffffffu) n = 0;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * kFramesPerWave;
  if (wave_base >= n) return;
  const uint32_t n_here = min((uint32_t)kFramesPerWave, n - wave_base);
  const uint8_t* wb = base + (uint64_t)wave_base * stride;
  uint32_t acc = 0;
  for (uint32_t b0 = 0; b0 < n_here; b0 += kBatch) {
    u32x4 w0s[kBatch], w1s[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      // one frame per load: its length is the same on every lane (scalar descriptor)
      const uint32_t nb = __builtin_amdgcn_readfirstlane(
          (b0 + j < n_here) ? min(lens[wave_base + b0 + j], min(stride, 2048u)) : 0u);
      const __amdgpu_buffer_rsrc_t rs = frame_rsrc(wb + (uint64_t)(b0 + j) * stride, nb);
      w0s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, 0, 0);
      w1s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, 1024 + lane * 16, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kBatch; ++j) acc ^= w0s[j].x ^ w0s[j].y ^ w0s[j].z ^ w0s[j].w ^ w1s[j].x ^ w1s[j].y ^ w1s[j].z ^ w1s[j].w;
  }
  if constexpr (STORE == 16) {
    if (lane < (int)n_here) {
      u32x4 r = {acc, acc ^ 1u, acc ^ 2u, acc ^ 3u};
      *reinterpret_cast<u32x4*>(sink + 4 * (uint64_t)(wave_base + lane)) = r;
    }
  } else {
    if (acc == 0x9E3779B9u) sink[blockIdx.x] = acc;
  }
}

// The production launch's arguments (strided_kargs) for the ceilings below.
int strided_args_calib(pn_ctx* ctx, const void* frames_dev, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                       void* results_dev, KArgs& a) {
  if (((uintptr_t)frames_dev & 15) || ((uintptr_t)results_dev & 15) || (slot_stride & 15) || slot_stride > 65536 ||
      slot_stride < frame_off + 96)
    return set_err(ctx, PN_EINVAL, "ceiling: layout contract");
  strided_kargs(a, frames_dev, results_dev, ctx->tbl_dev, ctx->mask, ctx->n_entries, ctx->max_conn, n, slot_stride, frame_off);
  if (!coop_layout(a)) return set_err(ctx, PN_EINVAL, "ceiling: needs the cooperative layout");
  return PN_OK;
}

} // namespace

extern "C" {

// Same-run ceiling for pn_classify (bench.py): the production kernel -- its window loads, stream
// loads, record stores, occupancy and workgroup order -- with the conn-table probe and the stream
// phase's lane reduction ablated.  Timing only: the records are wrong.  frame_off 2 or 18 (the
// MIS = 0 class, the bench's layout), cooperative layout.
int pn_calib_classify_ablated(pn_ctx* ctx, const void* frames_dev, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                              void* results_dev, void* stream) {
  if (!ctx || !ctx->tbl_dev || !frames_dev || !results_dev || n == 0 || (frame_off + 14) % 16 != 0)
    return set_err(ctx, PN_EINVAL, "pn_calib_classify_ablated: bad arguments");
  KArgs a;
  int rc = strided_args_calib(ctx, frames_dev, slot_stride, frame_off, n, results_dev, a);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_one<0, 1, kProdAbl | kAblNoProbe | kAblNoReduce>(a, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "pn_calib_classify_ablated launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

int pn_calib_slot_read(pn_ctx* ctx, const void* src_dev, uint32_t n_slots, uint32_t stride, uint32_t bytes,
                       int store_bytes, void* sink_dev, void* stream) {
  if (!ctx || !src_dev || !sink_dev || (stride & 15) || bytes > stride || bytes > 2048 || n_slots == 0)
    return set_err(ctx, PN_EINVAL, "pn_calib_slot_read: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t waves = (n_slots + kFramesPerWave - 1) / kFramesPerWave;
  const uint8_t* src = (const uint8_t*)src_dev;
  uint32_t* sink = (uint32_t*)sink_dev;
  switch (store_bytes) {
    case 16: hipLaunchKernelGGL((calib_slot_read_kernel<16>), dim3(waves), dim3(64), 0, s, src, n_slots, stride, bytes, sink); break;
    case 8: hipLaunchKernelGGL((calib_slot_read_kernel<8>), dim3(waves), dim3(64), 0, s, src, n_slots, stride, bytes, sink); break;
    default: hipLaunchKernelGGL((calib_slot_read_kernel<0>), dim3(waves), dim3(64), 0, s, src, n_slots, stride, bytes, sink);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "calib slot launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}


int pn_calib_slot_read_var(pn_ctx* ctx, const void* src_dev, uint32_t n_slots, uint32_t stride, const void* lens_dev,
                           int store_bytes, void* sink_dev, void* stream) {
  if (!ctx || !src_dev || !lens_dev || !sink_dev || (stride & 15) || n_slots == 0 ||
      (store_bytes != 0 && store_bytes != 16))
    return set_err(ctx, PN_EINVAL, "pn_calib_slot_read_var: bad arguments");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t waves = (n_slots + kFramesPerWave - 1) / kFramesPerWave;
  const uint8_t* src = (const uint8_t*)src_dev;
  const uint32_t* lens = (const uint32_t*)lens_dev;
  uint32_t* sink = (uint32_t*)sink_dev;
  if (store_bytes == 16)
    hipLaunchKernelGGL((calib_slot_read_var_kernel<16>), dim3(waves), dim3(64), 0, s, src, n_slots, stride, lens, sink);
  else
    hipLaunchKernelGGL((calib_slot_read_var_kernel<0>), dim3(waves), dim3(64), 0, s, src, n_slots, stride, lens, sink);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "calib slot var launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}


// pn_match_streams in either form (stream_match.hpp): 1 cooperative chunks through LDS, 0 one lane
// per frame; 2-4 the cooperative form with nt / sc0 / sc1 loads; 5 its loads alone (a ceiling); 6-8 the id
// stores write-through / nt (7: with nt loads).  A/B by scripts/bench_streams.py.
int pn_match_streams_variant(pn_ctx* ctx, const void* frames, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                             const pn_stream_filter* filters, uint32_t n_filters, uint32_t* stream_ids, void* stream,
                             int variant) {
  if (n == 0 || variant < 0 || variant > 40) return set_err(ctx, PN_EINVAL, "match variant: bad arguments");
  MatchArgs a;
  int rc = match_args(ctx, frames, slot_stride, frame_off, n, filters, n_filters, stream_ids, a);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (variant) {
    case 1: launch_match<kMatchProd, kMatchLoadAux>(a, frame_off, s); break; // round-3 production
    case 9: launch_match<1>(a, frame_off, s); break;     // cooperative, default-policy loads
    case 2: launch_match<1, 2>(a, frame_off, s); break;  // cooperative, nt loads
    case 3: launch_match<1, 1>(a, frame_off, s); break;  // cooperative, sc0 loads
    case 4: launch_match<1, 16>(a, frame_off, s); break; // cooperative, sc1 loads
    case 5: launch_match<2, kMatchLoadAux>(a, frame_off, s); break;     // timing-only ceiling: the same loads, no compare or store
    case 6: launch_match<1, 0, 16>(a, frame_off, s); break; // ids stored write-through (sc1)
    case 7: launch_match<1, 2, 16>(a, frame_off, s); break; // nt loads + sc1 id stores
    case 8: launch_match<1, 0, 2>(a, frame_off, s); break;  // ids stored nt
    // round 4: wave-ordered tile, mask compare, G groups per wave, W waves per workgroup
    // (match_streams_mask_kernel<.., G, .., OPT, W>); the odd-numbered-after-19 / 15-19 ids: loads + tile only
    case 10: launch_match_mask<1, kMatchLoadAux, 0, 4>(a, frame_off, s); break;
    case 11: launch_match_mask<2, kMatchLoadAux, 0, 4>(a, frame_off, s); break;
    case 12: launch_match_mask<4, kMatchLoadAux, 0, 4>(a, frame_off, s); break;
    case 13: launch_match_mask<1, kMatchLoadAux, 0, 1>(a, frame_off, s); break;
    case 14: launch_match_mask<2, kMatchLoadAux, 0, 1>(a, frame_off, s); break;
    case 15: launch_match_mask<1, kMatchLoadAux, 2, 4>(a, frame_off, s); break;  // timing only: 10's loads + tile
    case 16: launch_match_mask<2, kMatchLoadAux, 2, 4>(a, frame_off, s); break;  // 11's
    case 17: launch_match_mask<4, kMatchLoadAux, 2, 4>(a, frame_off, s); break;  // 12's
    case 18: launch_match_mask<1, kMatchLoadAux, 2, 1>(a, frame_off, s); break;  // 13's
    case 19: launch_match_mask<2, kMatchLoadAux, 2, 1>(a, frame_off, s); break;  // 14's
    case 20: launch_match_mask<4, kMatchLoadAux, 0, 1>(a, frame_off, s); break;
    case 21: launch_match_mask<4, kMatchLoadAux, 2, 1>(a, frame_off, s); break;  // 20's
    case 22: launch_match_mask<4, kMatchLoadAux, 0, 2>(a, frame_off, s); break;
    case 23: launch_match_mask<4, kMatchLoadAux, 2, 2>(a, frame_off, s); break;  // 22's
    case 24: launch_match_mask<8, kMatchLoadAux, 0, 4>(a, frame_off, s); break;
    case 25: launch_match_mask<8, kMatchLoadAux, 2, 4>(a, frame_off, s); break;  // 24's
    case 26: launch_match_mask<8, kMatchLoadAux, 0, 1>(a, frame_off, s); break;
    case 27: launch_match_mask<8, kMatchLoadAux, 2, 1>(a, frame_off, s); break;  // 26's
    case 28: launch_match_mask<2, kMatchLoadAux, 0, 2>(a, frame_off, s); break;
    case 29: launch_match_mask<2, kMatchLoadAux, 2, 2>(a, frame_off, s); break;  // 28's
    case 30: launch_match_mask<1, kMatchLoadAux, 4, 1>(a, frame_off, s); break;  // production + s_setprio 2 after the loads
    case 31: launch_match_mask<1, kMatchLoadAux, 8, 1>(a, frame_off, s); break;  // production, needed chunks only to the tile
    case 32: launch_match_mask<1, kMatchLoadAux, 12, 1>(a, frame_off, s); break; // both
    case 33: launch_match_mask<1, kMatchLoadAux, 16, 1>(a, frame_off, s); break; // production, and-compare form
    case 34: launch_match_mask<1, kMatchLoadAux, 32, 1>(a, frame_off, s); break; // timing only: no compare
    case 35: launch_match_mask<1, kMatchLoadAux, 64, 1>(a, frame_off, s); break; // timing only: no id store
    case 36: launch_match_mask<1, kMatchLoadAux, 128, 1>(a, frame_off, s); break; // production, nt id stores
    case 37: launch_match_mask<1, kMatchLoadAux, 256, 1>(a, frame_off, s); break; // production, masks loaded first
    case 38: launch_match_mask<1, kMatchLoadAux, 512, 1>(a, frame_off, s); break; // timing only: stores into 4 KiB
    case 39: launch_match_mask<1, kMatchLoadAux, 1024, 1>(a, frame_off, s); break; // no tile: quad DPP exchange
    case 40: launch_match_mask<1, kMatchLoadAux, 1024 | 2, 1>(a, frame_off, s); break; // 39's loads + exchange alone
    default: launch_match<0>(a, frame_off, s);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "match variant launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

int pn_test_spin_wait(const uint32_t* go_host, uint32_t* done_host, uint32_t max_ms, void* stream) {
  if (!go_host || !done_host || max_ms == 0 || max_ms > 10000)
    return set_err(nullptr, PN_EINVAL, "pn_test_spin_wait: go/done must be set, max_ms in [1, 10000]");
  int dev = 0, khz = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  if (e != hipSuccess || khz <= 0) return hip_err(nullptr, e, "wall clock rate");
  hipLaunchKernelGGL(spin_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, go_host, done_host,
                     (uint64_t)khz * max_ms);
  e = hipGetLastError();
  return e == hipSuccess ? PN_OK : hip_err(nullptr, e, "spin_wait launch");
}

int pn_test_doorbell_echo(const uint32_t* bell_host, uint32_t* echo_host, uint32_t max_idle_ms, int once, int sleep,
                          void* stream) {
  if (!bell_host || !echo_host || max_idle_ms == 0 || max_idle_ms > 10000)
    return set_err(nullptr, PN_EINVAL, "pn_test_doorbell_echo: bell/echo must be set, max_idle_ms in [1, 10000]");
  int dev = 0, khz = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  if (e != hipSuccess || khz <= 0) return hip_err(nullptr, e, "wall clock rate");
  hipLaunchKernelGGL(doorbell_echo_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, bell_host, echo_host,
                     (uint64_t)khz * max_idle_ms, (uint32_t)(once != 0), (uint32_t)(sleep != 0));
  e = hipGetLastError();
  return e == hipSuccess ? PN_OK : hip_err(nullptr, e, "doorbell_echo launch");
}

int pn_test_doorbell_echo_pipe(const uint32_t* bell_host, uint32_t* echo_host, uint32_t max_idle_ms, int depth,
                               uint32_t gap, void* stream) {
  if (!bell_host || !echo_host || max_idle_ms == 0 || max_idle_ms > 10000 || gap > 64 ||
      (depth != 1 && depth != 2 && depth != 4 && depth != 8))
    return set_err(nullptr, PN_EINVAL, "pn_test_doorbell_echo_pipe: bell/echo, max_idle_ms in [1, 10000], depth 1/2/4/8, gap <= 64");
  int dev = 0, khz = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  if (e != hipSuccess || khz <= 0) return hip_err(nullptr, e, "wall clock rate");
  const uint64_t t = (uint64_t)khz * max_idle_ms;
  const hipStream_t s = (hipStream_t)stream;
  switch (depth) {
    case 1: hipLaunchKernelGGL(doorbell_echo_pipe_kernel<1>, dim3(1), dim3(64), 0, s, bell_host, echo_host, t, gap); break;
    case 2: hipLaunchKernelGGL(doorbell_echo_pipe_kernel<2>, dim3(1), dim3(64), 0, s, bell_host, echo_host, t, gap); break;
    case 4: hipLaunchKernelGGL(doorbell_echo_pipe_kernel<4>, dim3(1), dim3(64), 0, s, bell_host, echo_host, t, gap); break;
    default: hipLaunchKernelGGL(doorbell_echo_pipe_kernel<8>, dim3(1), dim3(64), 0, s, bell_host, echo_host, t, gap);
  }
  e = hipGetLastError();
  return e == hipSuccess ? PN_OK : hip_err(nullptr, e, "doorbell_echo_pipe launch");
}

int pn_calib_stream_read(pn_ctx* ctx, const void* src_dev, uint64_t bytes, void* sink_dev, void* stream) {
  if (!ctx || !src_dev || !sink_dev || (bytes & 15) || ((uintptr_t)src_dev & 15))
    return set_err(ctx, PN_EINVAL, "pn_calib_stream_read: bad arguments");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  hipLaunchKernelGGL(calib_stream_read_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src_dev,
                     bytes / 16, (uint32_t*)sink_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "calib launch");
  pn_internal::note_stream(ctx, (hipStream_t)stream);
  return PN_OK;
}

} // extern "C"
