// udp_demux.hpp — the UDP demux path's kernels (device code + launch helper), included by udp_demux_kernel.hip.
// Internal linkage; one including translation unit.
#pragma once
// MI355X (gfx950) payload demux: the delivered datagrams of a classified ring (pn_udp_classify's records) grouped
// by subscription -- a stable sort by (sub_id, frame index) -- and packed into one buffer, each message 16-byte
// aligned and zero-padded, with pn_udp_gather's index arrays in that order and, per subscription, the first
// message and the first byte it owns.  A counting sort over frame tiles, then the gather's offset scan and copy over
// the grouped order.  Eight launches on the caller's stream:
//   count     one workgroup per tile of consecutive frames: the record load, the taken test, an LDS histogram of
//             the tile's messages per subscription (integer adds: their order does not matter); the row goes to the
//             tiles x n_subs matrix in ctx scratch.
//   cols      one thread per subscription walks its column over the tiles, coalesced across subscriptions, and
//             leaves the exclusive count before each tile; the column's total goes to the scratch sub_first.
//   subs      one workgroup scans the at most 4,096 totals: sub_first (scratch and output) and n_msgs.
//   place     one wave per tile, the tile's row + sub_first as running cursors in LDS, its frames in order 64 at a
//             time: a lane's rank among the wave's lanes with its sub_id comes from one ballot per key bit, j =
//             cursor + rank, the last peer advances the cursor.  pay_lens[j], sub_ids[j] and the source index at j.
//   sum       one wave per 256 messages in grouped order: their padded bytes (the source index back to the record,
//             the taken test again) summed into ctx scratch.
//   scan      one workgroup turns those sums into exclusive prefixes, 1,024 a pass with a carry; n_bytes, the total.
//   copy      one wave per 64 messages (a quarter of a chunk: the bytes of the quarters before it are summed again,
//             so that a batch with few messages still fills the chip): the offsets scanned in the wave (pay_offs,
//             the crossing message's n_fit), the payload bytes [0, 128) copied 8 lanes per message, the rest
//             streamed by the whole wave through a descriptor over exactly the message's dwords.  Whole aligned
//             16-byte non-temporal stores only.
//   subbytes  sub_bytes[s] = pay_offs[sub_first[s]], or n_bytes for a subscription past the last message.
// Nothing a record, an offset or the scratch holds can move a write outside the outputs: every j and every source
// index taken from scratch is clamped below n, every sub_id that indexes anything passed the taken test's
// sub_id < n_subs in the same kernel, and every message is checked against payload_cap with the offset the copy
// itself computed.  No atomic decides a position and no workgroup waits for another: the output is a function of
// the inputs alone.
// The copy is specialised on SH = (eth_mod16 + 42) % 4, the payload's place in its first dword (0 or 2).
#include <hip/hip_runtime.h>

#include "../../include/pollnet_amd.h"
#include "device_common.hpp"
#include "frame_pass.hpp"
#include "pn_internal.hpp"

namespace {

using namespace pn_dev;

constexpr uint32_t kUdHdr = 42;          // eth(14) + ip(20) + udp(8)
constexpr uint32_t kUdMaxTiles = 1024;   // rows of the count matrix: n_subs x 4 B each
constexpr uint32_t kUdMinTile = 256;     // frames per tile below kUdMinTile x kUdMaxTiles frames
constexpr int kUdCountThreads = 256;     // the count workgroup
constexpr int kUdColThreads = 64;        // subscriptions per cols workgroup
constexpr int kUdScanThreads = 1024;     // the subs workgroup (4 subscriptions a thread) and the scan's pass width
constexpr uint32_t kUdChunk = 4 * kWave; // messages per wave of sum, one scan entry; copy takes a quarter per wave
constexpr int kUdBatch = 4;              // long messages whose loads are in flight together (2 KiB each)
constexpr uint32_t kUdSfEntries = (PN_UDP_MAX_SUBS + 1 + 3) & ~3u;
static_assert(kUdScanThreads * 4 == PN_UDP_MAX_SUBS, "the subs workgroup takes four subscriptions a thread");

struct UdArgs {
  const uint8_t* frames; // strided: slot 0; indexed: base
  const uint64_t* offs;  // indexed: frame i's Ethernet header at frames + offs[i]; nullptr: strided
  const u32x4* results;
  uint8_t* pay;
  uint64_t cap;
  uint64_t* pay_offs;
  uint16_t* pay_lens;
  uint32_t* sub_ids;
  uint32_t* src_index; // may be nullptr
  uint32_t* sub_first;
  uint64_t* sub_bytes;
  pn_udp_gather_total* total;
  // ctx scratch (nullptr when n == 0)
  u32x4* hdr;     // {n_msgs, -, n_bytes (lo, hi)}
  uint32_t* sf;   // sub_first again: n_subs + 1 entries (no output is read back but pay_offs, by subbytes)
  uint64_t* wsum; // per chunk of kUdChunk messages: padded bytes, then the bytes before the chunk
  uint32_t* src;  // message j's frame index
  uint32_t* hist; // n_tiles rows of n_subs: messages of the tile per subscription, then those before the tile
  uint32_t n;
  uint32_t n_subs;
  uint32_t tile; // frames per tile
  uint32_t n_tiles;
  uint32_t n_chunks;
  uint32_t stride;
  uint32_t frame_off; // indexed: eth_mod16
  uint32_t avail;
};

__device__ __forceinline__ uint32_t ud_pad16(uint32_t len) { return (len + 15u) & ~15u; }

// Frame f's record (f < n) and whether it is taken: pn_udp_gather's test and sub_id < n_subs.  `src` is the address
// of the payload's first byte (0 when not taken).
__device__ __forceinline__ bool ud_taken(const UdArgs& a, uint32_t f, bool live, uint32_t& len, uint32_t& sub,
                                         uint64_t& src) {
  len = 0;
  sub = 0;
  src = 0;
  if (!live) return false;
  const u32x4 r = a.results[f];
  const uint32_t flags = r.w >> 16, plen = r.w & 0xffffu, poff = r.z >> 16;
  bool ok = PN_UDP_DELIVER(flags) && poff == kUdHdr && kUdHdr + plen <= a.avail && r.x < a.n_subs;
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
  src = (uint64_t)(uintptr_t)a.frames + eth + kUdHdr;
  return true;
}

// Message j of the grouped order (j < n_msgs when live): its frame from scratch, clamped, and that frame's record
// under the taken test again.
__device__ __forceinline__ bool ud_msg(const UdArgs& a, uint32_t j, bool live, uint32_t& len, uint64_t& src) {
  uint32_t i = 0, sub;
  if (live) i = min(a.src[j], a.n - 1u);
  return ud_taken(a, i, live, len, sub, src);
}

__device__ __forceinline__ uint32_t ud_n_msgs(const UdArgs& a) {
  return min((uint32_t)__builtin_amdgcn_readfirstlane(a.hdr[0].x), a.n);
}

// Inclusive prefix sum over the wave's lanes (every lane active).
__device__ __forceinline__ uint32_t ud_wave_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// ---- count: the tile's messages per subscription ----
__global__ __launch_bounds__(kUdCountThreads) void udp_demux_count_kernel(UdArgs a) {
  __shared__ uint32_t hist[PN_UDP_MAX_SUBS];
  const uint32_t t = threadIdx.x, tile = blockIdx.x;
  for (uint32_t s = t; s < a.n_subs; s += kUdCountThreads) hist[s] = 0u;
  __syncthreads();
  const uint32_t f0 = tile * a.tile, f1 = min(a.n, f0 + a.tile);
  for (uint32_t f = f0 + t; f < f1; f += kUdCountThreads) {
    uint32_t len, sub;
    uint64_t src;
    if (ud_taken(a, f, true, len, sub, src)) atomicAdd(&hist[sub], 1u); // sub < n_subs
  }
  __syncthreads();
  uint32_t* row = a.hist + (size_t)tile * a.n_subs;
  for (uint32_t s = t; s < a.n_subs; s += kUdCountThreads) row[s] = hist[s];
}

// ---- cols: per subscription, the messages before each tile; the column's total ----
__global__ __launch_bounds__(kUdColThreads) void udp_demux_cols_kernel(UdArgs a) {
  const uint32_t s = blockIdx.x * kUdColThreads + threadIdx.x;
  if (s >= a.n_subs) return;
  uint32_t* p = a.hist + s;
  uint32_t run = 0, t = 0;
  for (; t + 8 <= a.n_tiles; t += 8) { // eight independent loads in flight
    uint32_t c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = p[(size_t)(t + k) * a.n_subs];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      p[(size_t)(t + k) * a.n_subs] = run;
      run += c[k];
    }
  }
  for (; t < a.n_tiles; ++t) {
    const uint32_t c = p[(size_t)t * a.n_subs];
    p[(size_t)t * a.n_subs] = run;
    run += c;
  }
  a.sf[s] = run;
}

// ---- subs: sub_first and n_msgs from the column totals.  n == 0: zeroes every per-subscription entry and total ----
__global__ __launch_bounds__(kUdScanThreads) void udp_demux_subs_kernel(UdArgs a) {
  __shared__ uint32_t w_tot[kUdScanThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  uint32_t v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t s = 4u * t + k;
    v[k] = a.n && s < a.n_subs ? a.sf[s] : 0u;
    sum += v[k];
  }
  const uint32_t inc = ud_wave_scan(sum, lane);
  if (lane == kWave - 1) w_tot[wv] = inc;
  __syncthreads();
  uint32_t ex = inc - sum, tot = 0;
#pragma unroll
  for (int k = 0; k < kUdScanThreads / kWave; ++k) {
    if (k < wv) ex += w_tot[k];
    tot += w_tot[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t s = 4u * t + k;
    if (s < a.n_subs) {
      const uint32_t first = min(ex, a.n);
      if (a.n) a.sf[s] = first;
      a.sub_first[s] = first;
      if (!a.n) a.sub_bytes[s] = 0ull;
    }
    ex += v[k];
  }
  if (t == 0) {
    tot = min(tot, a.n);
    a.sub_first[a.n_subs] = tot;
    if (a.n) {
      a.sf[a.n_subs] = tot;
      a.hdr[0] = u32x4{tot, 0u, 0u, 0u};
    } else {
      a.sub_bytes[a.n_subs] = 0ull;
      pn_udp_gather_total z;
      z.n_bytes = 0;
      z.n_msgs = 0;
      z.n_fit = 0;
      *a.total = z;
    }
  }
}

// ---- place: every taken frame's j; the index entries at j ----
__global__ __launch_bounds__(kWave) void udp_demux_place_kernel(UdArgs a) {
  __shared__ uint32_t cur[PN_UDP_MAX_SUBS];
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  const uint32_t* row = a.hist + (size_t)tile * a.n_subs;
  for (uint32_t s = lane; s < a.n_subs; s += kWave) cur[s] = a.sf[s] + row[s];
  __syncthreads();
  const uint32_t key_bits = 32u - (uint32_t)__builtin_clz(a.n_subs | 1u); // covers every sub_id < n_subs
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t f0 = tile * a.tile, f1 = min(a.n, f0 + a.tile);
  for (uint32_t base = f0; base < f1; base += kWave) { // wave-uniform
    const uint32_t f = base + lane;
    uint32_t len, sub;
    uint64_t src;
    const bool taken = ud_taken(a, f, f < f1, len, sub, src);
    // the taken lanes with this lane's sub_id: every ballot with the whole wave active, the select afterwards
    uint64_t peers = __ballot(taken);
    for (uint32_t b = 0; b < key_bits; ++b) { // wave-uniform
      const bool bit = (sub >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below), cnt = (uint32_t)__popcll(peers);
    const uint32_t c = taken ? cur[sub] : 0u;
    __syncthreads(); // every read of the cursors before the last peers advance them
    if (taken && rank + 1u == cnt) cur[sub] = c + cnt;
    __syncthreads();
    if (taken) {
      const uint32_t j = min(c + rank, a.n - 1u); // j < n whatever the scratch holds
      a.pay_lens[j] = (uint16_t)len;
      a.sub_ids[j] = sub;
      a.src[j] = f;
      if (a.src_index) a.src_index[j] = f;
    }
  }
}

// ---- sum: the padded bytes of each chunk of messages in grouped order ----
__global__ __launch_bounds__(kWave) void udp_demux_sum_kernel(UdArgs a) {
  const uint32_t lane = threadIdx.x, chunk = blockIdx.x;
  const uint32_t n_msgs = ud_n_msgs(a);
  const uint32_t jb = chunk * kUdChunk;
  uint32_t bytes = 0; // at most 256 x 65,536
  if (jb < n_msgs) {  // wave-uniform
#pragma unroll
    for (uint32_t p = 0; p < kUdChunk / kWave; ++p) {
      const uint32_t j = jb + p * kWave + lane;
      uint32_t len;
      uint64_t src;
      const bool taken = ud_msg(a, j, j < n_msgs, len, src);
      bytes += taken ? ud_pad16(len) : 0u;
    }
  }
  bytes = ud_wave_scan(bytes, (int)lane);
  if (lane == kWave - 1) a.wsum[chunk] = bytes;
}

// ---- scan: the bytes before each chunk, in place; n_bytes, the total (n_fit = n_msgs until a message crosses) ----
__global__ __launch_bounds__(kUdScanThreads) void udp_demux_scan_kernel(UdArgs a) {
  __shared__ uint64_t w_bytes[kUdScanThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  uint64_t carry = 0;
  for (uint32_t c0 = 0; c0 < a.n_chunks; c0 += kUdScanThreads) { // uniform over the workgroup
    const uint32_t c = c0 + t;
    const bool in = c < a.n_chunks;
    const uint32_t e = in ? (uint32_t)a.wsum[c] : 0u; // at most 2^24: a wave's 64 sum below 2^32
    const uint32_t ib = ud_wave_scan(e, lane);
    if (lane == kWave - 1) w_bytes[wv] = ib;
    __syncthreads();
    uint64_t bb = carry, tb = 0;
#pragma unroll
    for (int k = 0; k < kUdScanThreads / kWave; ++k) {
      if (k < wv) bb += w_bytes[k];
      tb += w_bytes[k];
    }
    if (in) a.wsum[c] = bb + ib - e;
    carry += tb;
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t n_msgs = min(a.hdr[0].x, a.n);
    a.hdr[0] = u32x4{n_msgs, 0u, (uint32_t)carry, (uint32_t)(carry >> 32)};
    pn_udp_gather_total tot;
    tot.n_bytes = carry;
    tot.n_msgs = n_msgs;
    tot.n_fit = n_msgs;
    *a.total = tot;
  }
}

// ---- copy: pay_offs, n_fit, the payload bytes ----
template <int SH>
__global__ __launch_bounds__(kWave) void udp_demux_copy_kernel(UdArgs a) {
  static_assert(SH == 0 || SH == 2, "the payload starts 0 or 2 bytes into a dword");
  const int lane = threadIdx.x;
  const uint32_t n_msgs = ud_n_msgs(a);
  const uint32_t p0 = blockIdx.x * kWave; // the wave's 64 messages: a quarter of a chunk
  if (p0 >= n_msgs) return;               // wave-uniform
  const uint32_t chunk = p0 / kUdChunk;
  const uint64_t e = a.wsum[chunk];
  uint64_t byte_base =
      ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(e >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)e);
  // the padded bytes of the chunk's messages before the wave's own: at most three passes of 64 records
  for (uint32_t q0 = chunk * kUdChunk; q0 < p0; q0 += kWave) { // wave-uniform; q0 + lane < p0 < n_msgs
    uint32_t q_len;
    uint64_t q_src;
    const bool q_taken = ud_msg(a, q0 + lane, true, q_len, q_src);
    const uint32_t q_inc = ud_wave_scan(q_taken ? ud_pad16(q_len) : 0u, lane);
    byte_base += (uint32_t)__builtin_amdgcn_readlane(q_inc, kWave - 1);
  }

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

  {
    const uint32_t cnt = min((uint32_t)kWave, n_msgs - p0);
    const uint32_t j = p0 + lane;
    const bool has = (uint32_t)lane < cnt;
    uint32_t m_len;
    uint64_t m_src;
    const bool taken = ud_msg(a, j, has, m_len, m_src); // not taken: len 0, nothing copied
    const uint32_t pad = ud_pad16(m_len);
    const uint32_t inc = ud_wave_scan(pad, lane);
    const uint32_t m_boff = inc - pad;
    const uint64_t off = byte_base + m_boff;
    // copied only if it fits, by the offset computed here
    const bool fits = has && taken && off <= a.cap && pad <= a.cap - off;
    if (has) {
      a.pay_offs[j] = off;
      // the one message that starts at or below payload_cap and ends above it: the messages before it fit
      if (off <= a.cap && pad > a.cap - off) a.total->n_fit = j;
    }
    const uint32_t meta = m_len | (fits ? 0x10000u : 0u);

    // ---- short payloads: 8 lanes per message copy its first 128 B, 8 messages per pass ----
    for (uint32_t g = 0; g < cnt; g += 8) { // wave-uniform
      const uint32_t mi = g + ((uint32_t)lane >> 3);
      const int c = lane & 7, ml = (int)(mi & 63);
      const uint32_t meta_m = __shfl(meta, ml);
      const uint32_t b_m = __shfl(m_boff, ml);
      const uint32_t s_lo = __shfl((uint32_t)m_src, ml), s_hi = __shfl((uint32_t)(m_src >> 32), ml);
      const int len = (int)(meta_m & 0xffffu);
      if (!(mi < cnt && (meta_m & 0x10000u) && 16 * c < len)) continue;
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
    uint64_t need = __ballot(fits && m_len > 128);
    while (need) { // wave-uniform
      int lens_b[kUdBatch];
      uint8_t* dsts[kUdBatch];
      u32x4 w[kUdBatch][2];
      uint32_t we[kUdBatch][2];
      __amdgpu_buffer_rsrc_t rss[kUdBatch];
#pragma unroll
      for (int q = 0; q < kUdBatch; ++q) {
        const bool hasq = need != 0;
        const int fi = hasq ? __builtin_ctzll(need) : 0;
        if (hasq) need &= need - 1;
        const uint32_t ln = hasq ? (uint32_t)__builtin_amdgcn_readlane(m_len, fi) : 0u;
        lens_b[q] = (int)ln;
        const uint32_t s_lo = __builtin_amdgcn_readlane((uint32_t)m_src, fi);
        const uint32_t s_hi = __builtin_amdgcn_readlane((uint32_t)(m_src >> 32), fi);
        dsts[q] = a.pay + byte_base + (uint32_t)__builtin_amdgcn_readlane(m_boff, fi);
        // the message's dwords, exactly: past them a load returns zeros and fetches nothing
        rss[q] = frame_rsrc((const uint8_t*)((((uint64_t)s_hi << 32) | s_lo) - SH), ln ? ((SH + ln + 3) & ~3u) : 0u);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint32_t vo = 128 + 16 * lane + 1024 * s;
          w[q][s] = __builtin_amdgcn_raw_buffer_load_b128(rss[q], vo, 0, 0);
          we[q][s] = SH ? __builtin_amdgcn_raw_buffer_load_b32(rss[q], vo + 16, 0, 0) : 0u;
        }
      }
      __builtin_amdgcn_sched_barrier(0); // the batch's loads in flight before the first wait
#pragma unroll
      for (int q = 0; q < kUdBatch; ++q) {
        const int len = lens_b[q]; // 0 for an empty place of the batch: nothing below stores
        if (16 * (8 + lane) < len) emit(dsts[q], w[q][0], we[q][0], 8 + lane, len);
        if (16 * (72 + lane) < len) emit(dsts[q], w[q][1], we[q][1], 72 + lane, len);
        // jumbo slots: KiBs past the two above
        for (int c0 = 136; 16 * c0 < len; c0 += 64) {
          const uint32_t vo = 16 * (c0 + lane);
          const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rss[q], vo, 0, 0);
          const uint32_t xe = SH ? __builtin_amdgcn_raw_buffer_load_b32(rss[q], vo + 16, 0, 0) : 0u;
          if (16 * (c0 + lane) < len) emit(dsts[q], x, xe, c0 + lane, len);
        }
      }
    }
  }
}

// ---- subbytes: where each subscription's bytes start ----
__global__ __launch_bounds__(kUdCountThreads) void udp_demux_subbytes_kernel(UdArgs a) {
  const uint32_t s = blockIdx.x * kUdCountThreads + threadIdx.x;
  if (s > a.n_subs) return;
  const u32x4 h = a.hdr[0];
  const uint32_t n_msgs = min(h.x, a.n), first = a.sf[s];
  a.sub_bytes[s] = first >= n_msgs ? (((uint64_t)h.w << 32) | h.z) : a.pay_offs[first]; // first < n_msgs <= n
}

// ---- host side ----

// The launch plan of a batch of n frames: the tile (frames per count / place workgroup) keeps the count matrix at
// or below kUdMaxTiles rows; a chunk of kUdChunk messages is one entry of the offset scan.
struct UdPlan {
  uint32_t tile, n_tiles, n_chunks;
  size_t off_sf, off_wsum, off_src, off_hist, bytes; // the scratch: hdr at 0, every part 16-byte aligned
};

inline UdPlan ud_plan(uint32_t n, uint32_t n_subs) {
  UdPlan p = {};
  if (!n) return p;
  const uint32_t per = (n - 1) / kUdMaxTiles + 1;
  p.tile = per <= kUdMinTile ? kUdMinTile : (per + kWave - 1) / kWave * kWave;
  p.n_tiles = (n - 1) / p.tile + 1;
  p.n_chunks = (n - 1) / kUdChunk + 1;
  auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  p.off_sf = 16;
  p.off_wsum = p.off_sf + 4 * (size_t)kUdSfEntries;
  p.off_src = p.off_wsum + up16(8 * (size_t)p.n_chunks);
  p.off_hist = p.off_src + up16(4 * (size_t)n);
  p.bytes = p.off_hist + up16(4 * (size_t)p.n_tiles * n_subs);
  return p;
}

// ctx-owned scratch, grown on demand.  A call on another stream than the previous user is ordered after it on the
// device (pn_fence); growing waits on the host for that user before the old scratch is freed.
inline int ud_scratch(pn_ctx* ctx, size_t bytes, hipStream_t s) {
  if (bytes > ctx->ud_scratch_bytes) {
    if (ctx->ud_scratch) {
      const int rc = pn_internal::fence_host_wait(ctx, ctx->ud);
      if (rc) return rc;
      (void)hipFree(ctx->ud_scratch);
      ctx->ud_scratch = nullptr;
      ctx->ud_scratch_bytes = 0;
    }
    const size_t cap = bytes < ((size_t)1 << 20) ? ((size_t)1 << 20) : bytes;
    hipError_t e = hipMalloc(&ctx->ud_scratch, cap);
    if (e != hipSuccess) return pn_internal::hip_err(ctx, e, "hipMalloc(udp demux scratch)");
    ctx->ud_scratch_bytes = cap;
  }
  return pn_internal::fence_use(ctx, ctx->ud, s);
}

// The eight launches.  a.n == 0: subs alone zeroes the per-subscription arrays and the total on the stream.
inline int ud_launch(pn_ctx* ctx, UdArgs& a, hipStream_t s) {
  const UdPlan p = ud_plan(a.n, a.n_subs);
  a.tile = p.tile;
  a.n_tiles = p.n_tiles;
  a.n_chunks = p.n_chunks;
  if (a.n) {
    const int rc = ud_scratch(ctx, p.bytes, s);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)ctx->ud_scratch;
    a.hdr = (u32x4*)b;
    a.sf = (uint32_t*)(b + p.off_sf);
    a.wsum = (uint64_t*)(b + p.off_wsum);
    a.src = (uint32_t*)(b + p.off_src);
    a.hist = (uint32_t*)(b + p.off_hist);
    hipLaunchKernelGGL(udp_demux_count_kernel, dim3(a.n_tiles), dim3(kUdCountThreads), 0, s, a);
    hipLaunchKernelGGL(udp_demux_cols_kernel, dim3((a.n_subs - 1) / kUdColThreads + 1), dim3(kUdColThreads), 0, s, a);
  }
  hipLaunchKernelGGL(udp_demux_subs_kernel, dim3(1), dim3(kUdScanThreads), 0, s, a);
  if (a.n) {
    hipLaunchKernelGGL(udp_demux_place_kernel, dim3(a.n_tiles), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(udp_demux_sum_kernel, dim3(a.n_chunks), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(udp_demux_scan_kernel, dim3(1), dim3(kUdScanThreads), 0, s, a);
    if ((a.frame_off + kUdHdr) & 2) hipLaunchKernelGGL(udp_demux_copy_kernel<2>, dim3((a.n - 1) / kWave + 1), dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(udp_demux_copy_kernel<0>, dim3((a.n - 1) / kWave + 1), dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(udp_demux_subbytes_kernel, dim3(a.n_subs / kUdCountThreads + 1), dim3(kUdCountThreads), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pn_internal::hip_err(ctx, e, "udp_demux launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

} // namespace
