// udp_build.hpp — the UDP send path's kernel (device code + launch helper), included by udp_build_kernel.hip.
// Internal linkage; one including translation unit.
#pragma once
// MI355X (gfx950) datagram build: N messages in GPU-readable memory -> N wire-ready Ethernet / IPv4 / UDP frames
// in the slots of a TX ring.
//
// Reference: EfviUdpSender::write (Efvi.h:470-478) is update_udp_pkt (:611-621: tot_len, the IPv4 checksum from
// the sum cached at init, :405-411, and udp_len) plus one memcpy of the payload behind the 42 header bytes that
// init left in every pkt_buf (:436-440).  One sender object has one destination; here a launch builds for up to
// PN_UDP_MAX_CHANNELS destinations, each a 42-byte header template (pn_udp_set_channels), and may also compute the
// RFC 768 checksum Efvi leaves 0, summing the payload on the way as TcpConn::copyAndSum does (TcpConn.h:257-299).
//
// The kernel's main traffic is writes.  One wave takes `fpw` consecutive messages (frames_per_wave, xcd_group):
//   phase 0  lane = message: its offset, length and channel are read and checked; frame_lens is written (one
//            coalesced store).  A refused message takes no further part: nothing of it is read or written.
//   phase B  frames longer than their first 128-B block: the whole wave streams the rest of one frame at a
//            time, 1 KiB per step, four frames' loads in flight together.  The source is read through a buffer
//            descriptor that covers exactly the message's dwords (the hardware's per-dword range check returns
//            zeros past it and fetches nothing), one dwordx4 + one dword per lane at the dword-aligned address,
//            funnel-shifted (v_alignbyte) by the message's byte residue into the 16 bytes the lane stores.
//            PN_UB_CSUM sums those bytes as the datagram's words; the frame's total lands on its own lane.
//   phase A  8 lanes per frame, 8 frames per pass: lane c builds the c-th 16-B block of the slot's first 128 B
//            from the channel's template (with tot_len, the IPv4 checksum, udp_len and the UDP checksum put
//            in) and the first payload bytes, and stores it.  The header is written once, complete: the UDP
//            checksum needs the payload's sum, which is why phase B runs first.
// Every interior 16 bytes of a frame go out as one 16-byte store to a 16-byte-aligned address; the first block
// (when frame_off % 16 != 0) and the last go out as the dword / 2-byte / 1-byte stores that stay inside the
// frame.  Nothing outside [eth, eth + 42 + len) is written and no ring byte is read.  Global (per-lane pointer)
// stores: a per-lane buffer descriptor would be waterfalled (tx_fill.hpp).
// The kernel is specialised on DC = (frame_off + 42) % 16, the place in a 16-B block where the payload starts
// (8 classes, as the classify kernels are on (frame_off + 14) % 16), and on the mode.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/pollnet_amd.h"
#include "device_common.hpp"
#include "frame_pass.hpp"
#include "pn_internal.hpp"

namespace {

using namespace pn_dev;

constexpr int kUbHdr = 42;          // eth(14) + ip(20) + udp(8)
constexpr uint32_t kUbEntryDw = 12; // device table: one 48-B entry per channel

// The device table entry of a channel, built by pn_udp_set_channels (12 dwords):
//   bytes 0..41  the template with tot_len, the IPv4 checksum, udp_len and the UDP checksum zeroed (the kernel
//                ORs the built values in)
//   bytes 42..43 the UDP pseudo-header's constant words (src, dst, protocol 17, both ports), as the u16 words a
//                little-endian load gives, folded to 16 bits (never 0: the protocol word is in it)
//   bytes 44..47 Efvi's ipsum_cache after its first fold (Efvi.h:410), 17 bits: the header's ten words with
//                tot_len = check = 0
struct UbArgs {
  const uint8_t* pay;
  uint64_t pay_bytes;
  const uint64_t* offs;
  const uint16_t* lens;
  const uint32_t* chans; // nullptr: channel 0 for every message
  uint8_t* frames;
  uint16_t* frame_lens;
  const uint32_t* tbl;
  uint32_t n_chans;
  uint32_t n;
  uint32_t stride;
  uint32_t frame_off;
  uint32_t fpw;
};

// (1 << 8k) - 1 for k in [0, 4]: the low k bytes of a dword
__device__ __forceinline__ uint32_t low_bytes(int k) { return k >= 4 ? 0xFFFFFFFFu : ((1u << (8 * k)) - 1u); }
__device__ __forceinline__ int clamp04(int v) { return v < 0 ? 0 : (v > 4 ? 4 : v); }

// A 16-bit field at even frame position F into the output dword that starts at even frame position p.
__device__ __forceinline__ uint32_t put16(uint32_t dw, int p, int F, uint32_t v) {
  const int d = F - p;
  return d == 0 ? (dw | v) : d == 2 ? (dw | (v << 16)) : dw;
}

// The payload's share of an output dword at frame position p, as datagram words: bytes below 42 (header) and
// from `end` = 42 + len on (an odd tail's pad, the slot beyond) count as zero.
__device__ __forceinline__ uint32_t pay_sum(uint32_t dw, int p, int end, uint32_t acc) {
  const uint32_t m = low_bytes(clamp04(end - p)) & ~low_bytes(clamp04(kUbHdr - p));
  return dot2(dw & m, 0x10001u, acc);
}

// Bytes [lo, hi) of the 16-B block o[0..4) to dst (16-byte aligned); lo even, 0 <= lo < hi <= 16.  The widest
// stores that stay inside the range: the whole block, else per dword a dword, 2-byte and 1-byte store.
__device__ __forceinline__ void store_block(uint8_t* dst, const uint32_t (&o)[4], int lo, int hi) {
  if (lo == 0 && hi == 16) {
    const u32x4 v = {o[0], o[1], o[2], o[3]};
    // written once and not read again by the kernel: non-temporal, 7-8 % less kernel time than the default policy on
    // 1 Mi frames, 1472-B and 64-B payloads alike (non-temporal source loads measured 9-12 % slower)
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b0 = clamp04(lo - 4 * q), b1 = clamp04(hi - 4 * q);
    if (b0 >= b1) continue;
    uint8_t* d = dst + 4 * q;
    if (b0 == 0 && b1 == 4) {
      *reinterpret_cast<uint32_t*>(d) = o[q];
      continue;
    }
    if (b0 == 0) { // the low half: both bytes, or byte 0 alone
      if (b1 >= 2) *reinterpret_cast<uint16_t*>(d) = (uint16_t)o[q];
      else d[0] = (uint8_t)o[q];
    }
    if (b1 == 4) *reinterpret_cast<uint16_t*>(d + 2) = (uint16_t)(o[q] >> 16);
    else if (b1 == 3) d[2] = (uint8_t)(o[q] >> 16);
  }
}

// The sum of v over the wave (every lane active), wave-uniform.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v += dpp<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);  // quad_perm [2,3,0,1]
  v += dpp<0x141>(v); // row_half_mirror: the other quad of the 8
  v += dpp<0x128>(v); // row_ror:8: the other 8 of the row
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

constexpr int kUbBatch = 4; // phase B: frames whose loads are in flight together (2 KiB each)

template <int DC, int MODE>
__global__ __launch_bounds__(kWave) void udp_build_kernel(UbArgs a) {
  static_assert(DC % 2 == 0 && DC >= 0 && DC < 16 && (MODE == PN_UB_EFVI || MODE == PN_UB_PLAIN || MODE == PN_UB_CSUM),
                "alignment class and mode");
  constexpr int D = (DC + 6) & 15; // frame_off % 16: the frame starts D bytes into its first 16-B block
  constexpr bool CSUM = MODE == PN_UB_CSUM;
  const int lane = threadIdx.x;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  const bool live = (uint32_t)lane < n_here;
  const uint32_t f = wave_base + lane;

  // ---- phase 0: lane = message ----
  uint64_t off = 0;
  uint32_t len = 0, ch = 0;
  if (live) {
    off = a.offs[f];
    len = a.lens[f];
    if (a.chans) ch = a.chans[f];
  }
  // 42 + len fits the slot and frame_lens' 16 bits (so 28 + len fits tot_len), the channel exists, the payload
  // lies inside the buffer (64-bit)
  const bool ok = live && kUbHdr + len <= a.stride - a.frame_off && kUbHdr + len <= 65535 && ch < a.n_chans &&
                  off <= a.pay_bytes && len <= a.pay_bytes - off;
  if (live) a.frame_lens[f] = ok ? (uint16_t)(kUbHdr + len) : (uint16_t)0;
  if (!ok) {
    off = 0;
    len = 0;
    ch = 0;
  }
  // the 16-B block that holds the first frame's first byte
  uint8_t* const group = a.frames + (uint64_t)wave_base * a.stride + (a.frame_off & ~15u);

  // ---- phase B: the whole wave streams each long frame from its block 8 on ----
  uint32_t tail_sum = 0; // CSUM: on lane fi, the datagram-word sum of frame fi's payload past its first 128-B block
  uint64_t need = __ballot(ok && D + kUbHdr + len > 128);
  while (need) { // wave-uniform
    int fis[kUbBatch];
    uint32_t lens_b[kUbBatch], sh_b[kUbBatch], sums[kUbBatch];
    u32x4 w[kUbBatch][2];
    uint32_t we[kUbBatch][2];
    __amdgpu_buffer_rsrc_t rss[kUbBatch];
    uint32_t voffs[kUbBatch];
#pragma unroll
    for (int j = 0; j < kUbBatch; ++j) {
      const bool has = need != 0;
      const int fi = has ? __builtin_ctzll(need) : 0;
      if (has) need &= need - 1;
      fis[j] = has ? fi : -1;
      const uint32_t o_lo = __builtin_amdgcn_readlane((uint32_t)off, fi);
      const uint32_t o_hi = __builtin_amdgcn_readlane((uint32_t)(off >> 32), fi);
      const uint32_t ln = has ? (uint32_t)__builtin_amdgcn_readlane(len, fi) : 0u;
      lens_b[j] = ln;
      const uint32_t a3 = o_lo & 3;
      // the message's dwords, exactly: [off - a3, off + len) rounded up to a dword
      const uint8_t* src = a.pay + ((((uint64_t)o_hi << 32) | o_lo) - a3);
      rss[j] = frame_rsrc(src, ln ? ((a3 + ln + 3) & ~3u) : 0u);
      // output block c = 8 + lane holds frame bytes from p0 = 16 c - D, payload bytes from p0 - 42
      const uint32_t t0 = a3 + 128 + 16 * lane - D - kUbHdr;
      voffs[j] = t0 & ~3u;
      sh_b[j] = t0 & 3;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        w[j][s] = __builtin_amdgcn_raw_buffer_load_b128(rss[j], voffs[j] + 1024 * s, 0, 0);
        we[j][s] = __builtin_amdgcn_raw_buffer_load_b32(rss[j], voffs[j] + 1024 * s + 16, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0); // the batch's loads in flight before the first wait
#pragma unroll
    for (int j = 0; j < kUbBatch; ++j) {
      const int fi = fis[j];
      uint32_t sum = 0;
      if (fi >= 0) { // wave-uniform
        const int end = kUbHdr + (int)lens_b[j];
        uint8_t* slot = group + (uint64_t)fi * a.stride;
        const uint32_t sh = sh_b[j];
        auto emit = [&](const u32x4& x, uint32_t xe, int c) {
          const int p0 = 16 * c - D, hi = end - p0;
          if (hi <= 0) return;
          const uint32_t o[4] = {__builtin_amdgcn_alignbyte(x.y, x.x, sh), __builtin_amdgcn_alignbyte(x.z, x.y, sh),
                                 __builtin_amdgcn_alignbyte(x.w, x.z, sh), __builtin_amdgcn_alignbyte(xe, x.w, sh)};
          if constexpr (CSUM) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sum = pay_sum(o[q], p0 + 4 * q, end, sum);
          }
          store_block(slot + 16 * c, o, 0, hi < 16 ? hi : 16);
        };
        emit(w[j][0], we[j][0], 8 + lane);
        emit(w[j][1], we[j][1], 72 + lane);
        // jumbo slots: KiBs past the two above
        for (int c0 = 136; 16 * c0 - D < end; c0 += 64) {
          const uint32_t vo = voffs[j] + 16 * (c0 - 8);
          const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rss[j], vo, 0, 0);
          const uint32_t xe = __builtin_amdgcn_raw_buffer_load_b32(rss[j], vo + 16, 0, 0);
          emit(x, xe, c0 + lane);
        }
      }
      sums[j] = sum;
    }
    if constexpr (CSUM) {
#pragma unroll
      for (int j = 0; j < kUbBatch; ++j) {
        const uint32_t tot = wave_sum(sums[j]);
        if (lane == fis[j]) tail_sum = tot;
      }
    }
  }

  // ---- phase A: 8 lanes per frame build the slot's first 128-B block, header included ----
  const uint32_t meta = len | (ok ? 0x10000u : 0u);
  for (uint32_t g = 0; g < n_here; g += 8) { // wave-uniform
    const uint32_t m = g + ((uint32_t)lane >> 3);
    const int c = lane & 7;
    const int ml = (int)(m & 63);
    const uint32_t meta_m = __shfl(meta, ml);
    const uint32_t o_lo = __shfl((uint32_t)off, ml), o_hi = __shfl((uint32_t)(off >> 32), ml);
    const uint32_t ch_m = __shfl(ch, ml);
    const uint32_t tail_m = __shfl(tail_sum, ml);
    const uint32_t len_m = meta_m & 0xffff;
    const bool act = m < n_here && (meta_m & 0x10000u);
    const int p0 = 16 * c - D, end = kUbHdr + (int)len_m;
    const bool mine = act && p0 < end;

    uint32_t o[4] = {0u, 0u, 0u, 0u};
    uint32_t part = 0, cache = 0, pseudo = 0;
    if (mine) {
      uint32_t h[4] = {0u, 0u, 0u, 0u}, pl[4] = {0u, 0u, 0u, 0u};
      if (p0 < kUbHdr) { // template bytes [p0, p0 + 16): five dwords of the entry, realigned (p0 % 4 is 0 or 2)
        const uint32_t* te = a.tbl + (uint64_t)ch_m * kUbEntryDw;
        const int i0 = p0 >> 2;
        uint32_t t[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] = (i0 + k >= 0 && i0 + k < (int)kUbEntryDw) ? te[i0 + k] : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) h[q] = __builtin_amdgcn_alignbyte(t[q + 1], t[q], (uint32_t)p0 & 3);
        pseudo = te[10] >> 16;
        cache = te[11];
      }
      if (p0 + 16 > kUbHdr && len_m) { // payload bytes [p0 - 42, p0 - 26): the aligned dwords that hold them
        const uint32_t a3 = o_lo & 3;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pay + ((((uint64_t)o_hi << 32) | o_lo) - a3));
        const int t0 = (int)a3 + p0 - kUbHdr, j0 = t0 >> 2, lim = (int)(a3 + len_m);
        uint32_t v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = (j0 + k >= 0 && 4 * (j0 + k) < lim) ? src[j0 + k] : 0u; // only dwords holding a message byte
#pragma unroll
        for (int q = 0; q < 4; ++q) pl[q] = __builtin_amdgcn_alignbyte(v[q + 1], v[q], (uint32_t)t0 & 3);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = p0 + 4 * q;
        const uint32_t hm = low_bytes(clamp04(kUbHdr - p)); // the dword's header bytes (p even: none, two or all)
        o[q] = (h[q] & hm) | (pl[q] & ~hm);
        if constexpr (CSUM) part = pay_sum(o[q], p, end, part);
      }
    }
    // the fields every build writes (Efvi.h:615-620), as the u16 a little-endian store puts in network order
    const uint32_t tot_w = bswap16(28 + len_m), ulen_w = bswap16(8 + len_m);
    uint32_t ip_chk;
    if constexpr (MODE == PN_UB_EFVI) {
      uint32_t cc = cache + (cache >> 16); // Efvi.h:411: the carry stays in and is added again
      uint32_t ipsum = cc + tot_w;         // Efvi.h:617-619
      ipsum += ipsum >> 16;
      ip_chk = ~ipsum & 0xffff;
    } else {
      ip_chk = csum_fold(cache + tot_w);
    }
    uint32_t udp_chk = 0;
    if constexpr (CSUM) {
      uint32_t s = part; // the frame's 8 lanes: all 64 lanes are active here
      s += dpp<0xB1>(s);
      s += dpp<0x4E>(s);
      s += dpp<0x141>(s);
      // pseudo-header (src, dst, 0x0011, ulen) + ports + ulen + payload; below 2^32 for any 65,507-B payload
      udp_chk = csum_fold(s + tail_m + pseudo + 2 * ulen_w);
      if (udp_chk == 0) udp_chk = 0xffff;
    }
    if (mine) {
      if (p0 < kUbHdr) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = p0 + 4 * q;
          o[q] = put16(o[q], p, 16, tot_w);
          o[q] = put16(o[q], p, 24, ip_chk);
          o[q] = put16(o[q], p, 38, ulen_w);
          o[q] = put16(o[q], p, 40, udp_chk);
        }
      }
      const int hi = end - p0;
      store_block(group + (uint64_t)m * a.stride + 16 * c, o, c == 0 ? D : 0, hi < 16 ? hi : 16);
    }
  }
}

// ---- host side ----

template <int MODE>
void ub_launch_mode(const UbArgs& a, hipStream_t s) {
  const dim3 grid((a.n + a.fpw - 1) / a.fpw), block(kWave);
  for_mis(a.frame_off, [&](auto mis) { // (frame_off + 42) % 16 = ((frame_off + 14) % 16 + 12) % 16
    constexpr int DC = (decltype(mis)::value + 12) & 15;
    hipLaunchKernelGGL((udp_build_kernel<DC, MODE>), grid, block, 0, s, a);
  });
}

inline void ub_launch(const UbArgs& a, uint32_t mode, hipStream_t s) {
  switch (mode) {
    case PN_UB_EFVI: return ub_launch_mode<PN_UB_EFVI>(a, s);
    case PN_UB_PLAIN: return ub_launch_mode<PN_UB_PLAIN>(a, s);
    default: return ub_launch_mode<PN_UB_CSUM>(a, s);
  }
}

} // namespace
