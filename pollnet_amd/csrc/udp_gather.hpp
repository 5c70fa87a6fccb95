// udp_gather.hpp — the UDP gather path's kernels (device code + launch helper), included by udp_gather_kernel.hip.
// Internal linkage; one including translation unit.
#pragma once
// MI355X (gfx950) payload gather: the delivered datagrams of a classified ring (pn_udp_classify's records) packed
// in arrival order into one contiguous buffer, each message 16-byte aligned and zero-padded, with the index arrays
// pn_udp_build takes (pay_offs, pay_lens, chan_ids = sub_ids).  The inverse of udp_build.hpp: the same bytes, the
// other direction -- reads through a wave-uniform descriptor over exactly the message's dwords, funnel-shifted by
// the source's byte residue, and nothing but whole aligned 16-byte non-temporal stores.
//
// Where a message lands depends on every frame before it, so the work is three launches on the caller's stream:
//   count  lane = frame (frames_per_wave, xcd_group, as the classify and build kernels): one 16-byte record load,
//          the taken test, a wave reduction; {messages, padded bytes} of the wave go to ctx scratch (16 B a wave).
//   scan   one workgroup turns the wave entries into exclusive prefixes in place, 1,024 a pass with a carry, writes
//          pn_udp_gather_total, and finds n_fit in the one wave whose bytes cross payload_cap.
//   copy   the count's waves again: every lane repeats the taken test, the wave's messages are compacted onto its
//          first lanes (ballot ranks, one ds_permute), their byte offsets scanned in the wave and added to the
//          wave's base.  The index entries go out at consecutive j.  Payload bytes [0, 128) are copied 8 lanes per
//          message, 8 messages per pass; the rest is streamed by the whole wave, 1 KiB per step, four messages'
//          loads in flight together.
// Nothing a record or an offset holds can move a write outside the outputs: a wave's message base is clamped to its
// first frame index (j <= i < n), and every message is checked against payload_cap with the offset the copy itself
// computed.  No atomics, no workgroup waits for another: the output is a function of the inputs alone.
// The copy is specialised on SH = (eth_mod16 + 42) % 4, the payload's place in its first dword (0 or 2).
#include <hip/hip_runtime.h>

#include "../../include/pollnet_amd.h"
#include "device_common.hpp"
#include "frame_pass.hpp"
#include "pn_internal.hpp"

namespace {

using namespace pn_dev;

constexpr uint32_t kUgHdr = 42;      // eth(14) + ip(20) + udp(8)
constexpr int kUgScanThreads = 1024; // wave entries the scan workgroup takes per pass
constexpr int kUgBatch = 4;          // long messages whose loads are in flight together (2 KiB each)

// One entry of the ctx scratch per wave.  After the count: {messages, padded bytes, -, -}.  After the scan:
// {messages before the wave, -, padded bytes before the wave (lo, hi)}.
struct UgArgs {
  const uint8_t* frames;  // strided: slot 0; indexed: base
  const uint64_t* offs;   // indexed: frame i's Ethernet header at frames + offs[i]; nullptr: strided
  const u32x4* results;
  uint8_t* pay;
  uint64_t cap;
  uint64_t* pay_offs;
  uint16_t* pay_lens;
  uint32_t* sub_ids;
  uint32_t* src_index; // may be nullptr
  u32x4* scratch;
  pn_udp_gather_total* total;
  uint32_t n;
  uint32_t n_waves;
  uint32_t stride;
  uint32_t frame_off; // indexed: eth_mod16
  uint32_t avail;
  uint32_t fpw;
};

__device__ __forceinline__ uint32_t ug_pad16(uint32_t len) { return (len + 15u) & ~15u; }

// Frame f's record and whether it is taken: PN_UDP_DELIVER, payload_off == 42, 42 + payload_len <= avail and, for
// an indexed call, an offset in the call's class (the classify gives every other offset PN_UF_BADOFF, never
// DELIVER).  `src` is the address of the payload's first byte (0 when not taken).
__device__ __forceinline__ bool ug_taken(const UgArgs& a, uint32_t f, bool live, uint32_t& len, uint32_t& sub,
                                         uint64_t& src) {
  len = 0;
  sub = 0;
  src = 0;
  if (!live) return false;
  const u32x4 r = a.results[f];
  const uint32_t flags = r.w >> 16, plen = r.w & 0xffffu, poff = r.z >> 16;
  bool ok = PN_UDP_DELIVER(flags) && poff == kUgHdr && kUgHdr + plen <= a.avail;
  uint64_t eth;
  if (a.offs) { // wave-uniform
    const uint64_t o = a.offs[f];
    ok = ok && (o & 15u) == a.frame_off;
    eth = o;
  } else {
    eth = (uint64_t)f * a.stride + a.frame_off;
  }
  if (!ok) return false;
  len = plen;
  sub = r.x;
  src = (uint64_t)(uintptr_t)a.frames + eth + kUgHdr;
  return true;
}

// Inclusive prefix sum over the wave's lanes (every lane active).
__device__ __forceinline__ uint32_t ug_wave_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// The sum of v over the wave (every lane active), wave-uniform.
__device__ __forceinline__ uint32_t ug_wave_sum(uint32_t v) {
  v += dpp<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);  // quad_perm [2,3,0,1]
  v += dpp<0x141>(v); // row_half_mirror: the other quad of the 8
  v += dpp<0x128>(v); // row_ror:8: the other 8 of the row
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

// The wave's messages in frame order on its first lanes.  Lane r < cnt gets message r: its length, subscription,
// source address, source lane and byte offset inside the wave's output (the padded lengths before it).
struct UgMsg {
  uint32_t cnt;
  uint32_t len, sub, boff, sl;
  uint64_t src;
};

__device__ __forceinline__ UgMsg ug_compact(bool taken, uint32_t len, uint32_t sub, uint64_t src, int lane) {
  UgMsg m;
  const uint64_t tk = __ballot(taken);
  m.cnt = (uint32_t)__popcll(tk);
  const uint32_t rank = (uint32_t)__popcll(tk & ((1ull << lane) - 1ull));
  // a permutation of the lanes: the taken ones first, in order, then the others
  const uint32_t dest = taken ? rank : m.cnt + ((uint32_t)lane - rank);
  m.sl = (uint32_t)__builtin_amdgcn_ds_permute((int)(dest * 4), lane);
  const bool has = (uint32_t)lane < m.cnt;
  // every shuffle with the whole wave active (a lane that is not reads as zero): select afterwards
  const uint32_t len_r = __shfl(len, m.sl);
  m.len = has ? len_r : 0u;
  m.sub = __shfl(sub, m.sl);
  const uint32_t lo = __shfl((uint32_t)src, m.sl), hi = __shfl((uint32_t)(src >> 32), m.sl);
  m.src = has ? (((uint64_t)hi << 32) | lo) : 0ull;
  const uint32_t pad = ug_pad16(m.len);
  m.boff = ug_wave_scan(pad, lane) - pad;
  return m;
}

// ---- count: {messages, padded bytes} per wave ----
__global__ __launch_bounds__(kWave) void udp_gather_count_kernel(UgArgs a) {
  const int lane = threadIdx.x;
  const uint32_t group = xcd_group(blockIdx.x, gridDim.x);
  const uint32_t wave_base = group * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  uint32_t len, sub;
  uint64_t src;
  const bool taken = ug_taken(a, wave_base + lane, (uint32_t)lane < n_here, len, sub, src);
  const uint32_t msgs = (uint32_t)__popcll(__ballot(taken));
  const uint32_t bytes = ug_wave_sum(taken ? ug_pad16(len) : 0u); // at most 64 x 65,536
  if (lane == 0) a.scratch[group] = u32x4{msgs, bytes, 0u, 0u};
}

// ---- scan: exclusive prefixes in place, the total, n_fit ----
__global__ __launch_bounds__(kUgScanThreads) void udp_gather_scan_kernel(UgArgs a) {
  __shared__ uint32_t w_msgs[kUgScanThreads / kWave];
  __shared__ uint64_t w_bytes[kUgScanThreads / kWave];
  __shared__ uint32_t cross_wave, cross_msgs;
  __shared__ uint64_t cross_bytes;
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  if (t == 0) cross_wave = 0xFFFFFFFFu;
  __syncthreads();
  uint32_t carry_m = 0;
  uint64_t carry_b = 0;
  for (uint32_t w0 = 0; w0 < a.n_waves; w0 += kUgScanThreads) { // uniform over the workgroup
    const uint32_t w = w0 + t;
    const bool in = w < a.n_waves;
    u32x4 e = {0u, 0u, 0u, 0u};
    if (in) e = a.scratch[w];
    const uint32_t im = ug_wave_scan(e.x, lane); // at most 64 per entry: no overflow below 2^32 frames
    // bytes: two 32-bit scans would need a carry; a wave's 64 entries of at most 2^22 each sum below 2^32
    const uint32_t ib = ug_wave_scan(e.y, lane);
    if (lane == kWave - 1) {
      w_msgs[wv] = im;
      w_bytes[wv] = ib;
    }
    __syncthreads();
    uint32_t bm = carry_m, tm = 0;
    uint64_t bb = carry_b, tb = 0;
#pragma unroll
    for (int k = 0; k < kUgScanThreads / kWave; ++k) {
      if (k < wv) {
        bm += w_msgs[k];
        bb += w_bytes[k];
      }
      tm += w_msgs[k];
      tb += w_bytes[k];
    }
    const uint32_t ex_m = bm + im - e.x;
    const uint64_t ex_b = bb + ib - e.y;
    if (in) {
      a.scratch[w] = u32x4{ex_m, 0u, (uint32_t)ex_b, (uint32_t)(ex_b >> 32)};
      // the one wave whose bytes cross payload_cap: its base fits, its end does not (ends never descend)
      if (ex_b <= a.cap && ex_b + e.y > a.cap) {
        cross_wave = w;
        cross_msgs = ex_m;
        cross_bytes = ex_b;
      }
    }
    carry_m += tm;
    carry_b += tb;
    __syncthreads();
  }
  if (wv != 0) return;
  // n_fit: every message when all fit, else the messages before the crossing wave and those of it that end
  // at or below payload_cap (the wave's frames again, by the workgroup's first wave)
  uint32_t n_fit = carry_m;
  const uint32_t cw = cross_wave;
  if (cw != 0xFFFFFFFFu) { // wave-uniform
    const uint32_t wave_base = cw * a.fpw;
    const uint32_t n_here = wave_base < a.n ? min(a.fpw, a.n - wave_base) : 0u;
    uint32_t len, sub;
    uint64_t src;
    const bool taken = ug_taken(a, wave_base + lane, (uint32_t)lane < n_here, len, sub, src);
    const uint32_t pad = taken ? ug_pad16(len) : 0u;
    const uint32_t end = ug_wave_scan(pad, lane);
    n_fit = cross_msgs + (uint32_t)__popcll(__ballot(taken && cross_bytes + end <= a.cap));
  }
  if (lane == 0) {
    pn_udp_gather_total tot;
    tot.n_bytes = carry_b;
    tot.n_msgs = carry_m;
    tot.n_fit = n_fit;
    *a.total = tot;
  }
}

// ---- copy ----
template <int SH>
__global__ __launch_bounds__(kWave) void udp_gather_copy_kernel(UgArgs a) {
  static_assert(SH == 0 || SH == 2, "the payload starts 0 or 2 bytes into a dword");
  const int lane = threadIdx.x;
  const uint32_t group = xcd_group(blockIdx.x, gridDim.x);
  const uint32_t wave_base = group * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);

  // ---- offsets and index arrays ----
  uint32_t len0, sub0;
  uint64_t src0;
  const bool taken = ug_taken(a, wave_base + lane, (uint32_t)lane < n_here, len0, sub0, src0);
  const UgMsg m = ug_compact(taken, len0, sub0, src0, lane);
  if (m.cnt == 0) return; // wave-uniform
  const u32x4 e = a.scratch[group];
  const uint32_t e_m = __builtin_amdgcn_readfirstlane(e.x);
  // j <= i whatever the scratch holds: the wave's first message is not above its first frame
  const uint32_t msg_base = min(e_m, wave_base);
  const uint64_t byte_base =
      ((uint64_t)__builtin_amdgcn_readfirstlane(e.w) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(e.z);
  const bool has = (uint32_t)lane < m.cnt;
  const uint64_t off = byte_base + m.boff;
  const uint32_t pad = ug_pad16(m.len);
  // copied only if it fits, by the offset computed here
  const bool fits = has && off <= a.cap && pad <= a.cap - off;
  if (has) {
    const uint32_t j = msg_base + lane;
    a.pay_offs[j] = off;
    a.pay_lens[j] = (uint16_t)m.len;
    a.sub_ids[j] = m.sub;
    if (a.src_index) a.src_index[j] = wave_base + m.sl;
  }
  const uint32_t meta = m.len | (fits ? 0x10000u : 0u);

  // One 16-B output block: payload bytes [16c, 16c + 16) from the five dwords x, xe that hold them, zeros from len on
  auto emit = [&](uint8_t* dst, const u32x4& x, uint32_t xe, int c, int len) {
    uint32_t o[4];
    if constexpr (SH == 0) {
      o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w;
    } else {
      o[0] = __builtin_amdgcn_alignbyte(x.y, x.x, SH), o[1] = __builtin_amdgcn_alignbyte(x.z, x.y, SH);
      o[2] = __builtin_amdgcn_alignbyte(x.w, x.z, SH), o[3] = __builtin_amdgcn_alignbyte(xe, x.w, SH);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int k = len - (16 * c + 4 * q);
      k = k < 0 ? 0 : (k > 4 ? 4 : k);
      o[q] &= k >= 4 ? 0xFFFFFFFFu : ((1u << (8 * k)) - 1u);
    }
    const u32x4 v = {o[0], o[1], o[2], o[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst + 16 * c));
  };

  // ---- short payloads: 8 lanes per message copy its first 128 B, 8 messages per pass ----
  for (uint32_t g = 0; g < m.cnt; g += 8) { // wave-uniform
    const uint32_t mi = g + ((uint32_t)lane >> 3);
    const int c = lane & 7, ml = (int)(mi & 63);
    const uint32_t meta_m = __shfl(meta, ml);
    const uint32_t b_m = __shfl(m.boff, ml);
    const uint32_t s_lo = __shfl((uint32_t)m.src, ml), s_hi = __shfl((uint32_t)(m.src >> 32), ml);
    const int len = (int)(meta_m & 0xffffu);
    if (!(mi < m.cnt && (meta_m & 0x10000u) && 16 * c < len)) continue;
    // the aligned dwords that hold a message byte, and no other
    const uint32_t* s = reinterpret_cast<const uint32_t*>((((uint64_t)s_hi << 32) | s_lo) - SH);
    const int lim = SH + len;
    uint32_t v[5];
#pragma unroll
    for (int k = 0; k < (SH ? 5 : 4); ++k) v[k] = 4 * (4 * c + k) < lim ? s[4 * c + k] : 0u;
    if constexpr (SH == 0) v[4] = 0u;
    emit(a.pay + byte_base + b_m, u32x4{v[0], v[1], v[2], v[3]}, v[4], c, len);
  }

  // ---- long payloads: the whole wave streams each message from byte 128 on ----
  uint64_t need = __ballot(fits && m.len > 128);
  while (need) { // wave-uniform
    int lens_b[kUgBatch];
    uint8_t* dsts[kUgBatch];
    u32x4 w[kUgBatch][2];
    uint32_t we[kUgBatch][2];
    __amdgpu_buffer_rsrc_t rss[kUgBatch];
#pragma unroll
    for (int j = 0; j < kUgBatch; ++j) {
      const bool hasj = need != 0;
      const int fi = hasj ? __builtin_ctzll(need) : 0;
      if (hasj) need &= need - 1;
      const uint32_t ln = hasj ? (uint32_t)__builtin_amdgcn_readlane(m.len, fi) : 0u;
      lens_b[j] = (int)ln;
      const uint32_t s_lo = __builtin_amdgcn_readlane((uint32_t)m.src, fi);
      const uint32_t s_hi = __builtin_amdgcn_readlane((uint32_t)(m.src >> 32), fi);
      dsts[j] = a.pay + byte_base + (uint32_t)__builtin_amdgcn_readlane(m.boff, fi);
      // the message's dwords, exactly: past them a load returns zeros and fetches nothing
      rss[j] = frame_rsrc((const uint8_t*)((((uint64_t)s_hi << 32) | s_lo) - SH), ln ? ((SH + ln + 3) & ~3u) : 0u);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint32_t vo = 128 + 16 * lane + 1024 * s;
        w[j][s] = __builtin_amdgcn_raw_buffer_load_b128(rss[j], vo, 0, 0);
        we[j][s] = SH ? __builtin_amdgcn_raw_buffer_load_b32(rss[j], vo + 16, 0, 0) : 0u;
      }
    }
    __builtin_amdgcn_sched_barrier(0); // the batch's loads in flight before the first wait
#pragma unroll
    for (int j = 0; j < kUgBatch; ++j) {
      const int len = lens_b[j]; // 0 for an empty place of the batch: nothing below stores
      if (16 * (8 + lane) < len) emit(dsts[j], w[j][0], we[j][0], 8 + lane, len);
      if (16 * (72 + lane) < len) emit(dsts[j], w[j][1], we[j][1], 72 + lane, len);
      // jumbo slots: KiBs past the two above
      for (int c0 = 136; 16 * c0 < len; c0 += 64) {
        const uint32_t vo = 16 * (c0 + lane);
        const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rss[j], vo, 0, 0);
        const uint32_t xe = SH ? __builtin_amdgcn_raw_buffer_load_b32(rss[j], vo + 16, 0, 0) : 0u;
        if (16 * (c0 + lane) < len) emit(dsts[j], x, xe, c0 + lane, len);
      }
    }
  }
}

// ---- host side ----

// ctx-owned wave entries, grown on demand.  A call on another stream than the previous user is ordered after it on
// the device (pn_fence); growing waits on the host for that user before the old scratch is freed.
inline int ug_scratch(pn_ctx* ctx, uint32_t n_waves, hipStream_t s) {
  if (n_waves > ctx->ug_scratch_n) {
    if (ctx->ug_scratch) {
      const int rc = pn_internal::fence_host_wait(ctx, ctx->ug);
      if (rc) return rc;
      (void)hipFree(ctx->ug_scratch);
      ctx->ug_scratch = nullptr;
      ctx->ug_scratch_n = 0;
    }
    const uint32_t cap = n_waves < (1u << 14) ? (1u << 14) : n_waves;
    hipError_t e = hipMalloc(&ctx->ug_scratch, (size_t)cap * sizeof(u32x4));
    if (e != hipSuccess) return pn_internal::hip_err(ctx, e, "hipMalloc(udp gather scratch)");
    ctx->ug_scratch_n = cap;
  }
  return pn_internal::fence_use(ctx, ctx->ug, s);
}

// The three launches.  a.n == 0: the scan alone, over no waves, zeroes the total on the stream.
inline int ug_launch(pn_ctx* ctx, UgArgs& a, hipStream_t s) {
  a.fpw = frames_per_wave(a.n);
  a.n_waves = a.n ? (a.n - 1) / a.fpw + 1 : 0;
  a.scratch = nullptr;
  if (a.n) {
    const int rc = ug_scratch(ctx, a.n_waves, s);
    if (rc) return rc;
    a.scratch = (u32x4*)ctx->ug_scratch;
    hipLaunchKernelGGL(udp_gather_count_kernel, dim3(a.n_waves), dim3(kWave), 0, s, a);
  }
  hipLaunchKernelGGL(udp_gather_scan_kernel, dim3(1), dim3(kUgScanThreads), 0, s, a);
  if (a.n) {
    if ((a.frame_off + kUgHdr) & 2) hipLaunchKernelGGL(udp_gather_copy_kernel<2>, dim3(a.n_waves), dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(udp_gather_copy_kernel<0>, dim3(a.n_waves), dim3(kWave), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pn_internal::hip_err(ctx, e, "udp_gather launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

} // namespace
