// udp_indexed.hpp — the indexed UDP receive kernel (device code + launch helper) behind pn_udp_classify_indexed:
// pn_udp_classify's record for frames that lie wherever an RX event, a packet-mmap block or a packed capture put
// them -- frame i's Ethernet header at base + offsets[i] -- as pn_classify_indexed is to pn_classify.  The ring
// EfviUdpReceiver reads from (Efvi.h:140, 194-200: pkt_bufs + id * PKT_BUF_SIZE + 64 + prefix_len) is classified
// where the NIC wrote it, in event order.
// Included by udp_indexed_kernel.hip only; everything is internal linkage.  The subscription table, its hash and
// the probe are udp_classify.hpp's (included, unchanged: the strided kernels keep their code).
//
// Same execution model as the strided kernel: one wave per frames_per_wave(n) frames, one-wave workgroups in XCD
// order, specialised on MIS = (eth_mod16 + 14) % 16.
//  phase 1  lane f loads offsets[f].  An offset outside the launch's class is not parsed (PN_UF_BADOFF), none of its
//           bytes are read.  The others get their header window from base + offsets[f] + 14 - MIS: 8 lanes per
//           frame load its 128-B window block into the LDS tile when every frame of the wave has that block inside
//           [base, eth + avail) (the RX kernel's indexed form, rx_classify.hpp), else each lane its own window, no
//           byte at or past avail used.  Field decode and subscription probe as the strided kernel.
//  phase 2  the summed frames alone, through the frame pass's per-frame-address stream: every frame of the wave
//           (full-size: every load issued; else the skipping form), or the summed ones compacted onto the first
//           lanes; a wave with none streams nothing.
//  phase 3  as the strided kernel; one coalesced 16-B record per lane, in offsets order.
#pragma once

#include "udp_classify.hpp"

namespace {

struct UdpIdxArgs : UdpArgs { // frames = base, avail = the call's; stride and ipa_off are 0
  const uint64_t* offs;
};

// The cooperative window blocks are loaded at the default cache policy, as the RX kernel's indexed launches load
// them (rx_classify.hpp, kIdxWin): in a packed capture a frame's last line is the next frame's window line.
template <int MIS, bool HO>
__global__ __launch_bounds__(kWave, 4) void udp_indexed_kernel(UdpIdxArgs a) {
  static_assert(MIS + 28 <= kWinBytes, "window must cover ip .. ip+28");
  const int lane = threadIdx.x;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t f = wave_base + lane;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  const bool live = (uint32_t)lane < n_here;

  // ---- phase 1 ----
  Window h;
#pragma unroll
  for (int q = 0; q < 4 * kWinChunks; ++q) h.d[q] = 0;
  uint32_t ether_type = 0;
  const uint64_t o = live ? a.offs[f] : 0;
  const bool bad_off = live && ((o + 14) & 15) != (uint64_t)MIS;
  const bool use = live && !bad_off;
  const uint8_t* win = a.frames + o + 14 - MIS; // ip - MIS; dereferenced by `use` lanes only
  // every frame of the wave has its window block (the 16-B chunk before the window, and the window) 16-B aligned
  // inside [base, eth + avail)
  const bool elig = !use || ((((uintptr_t)win & 15u) == 0) && o + 14 >= (uint64_t)(MIS + 16) &&
                             (uint32_t)(14 - MIS + kWinBytes) <= a.avail);
  if (__all(elig)) {
    __shared__ uint64_t line_addr[kFramesPerWave];
    line_addr[lane] = use ? (uint64_t)(win - 16) : 0ull;
    __syncthreads();
    u32x4* tile = coop_tile();
    // all 8 loads in flight before the first LDS write: a part that is not needed reads its block's first chunk
    // instead (a line the same instruction fetches anyway; for an unused row, the first used frame's block) and is
    // zeroed, rather than a branch around it
    const uint64_t used = __ballot(use);
    const uint32_t l0 = used ? (uint32_t)__builtin_ctzll(used) : 0u;
    const uint64_t wb = (uint64_t)(win - 16);
    const uint64_t safe = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(wb >> 32), l0) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((uint32_t)wb, l0);
    u32x4 v[8];
    bool need[8];
    const u32x4* src[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      const uint64_t la = line_addr[r];
      need[i] = la && block_part_needed<MIS>((uint32_t)la, part);
      src[i] = need[i] ? reinterpret_cast<const u32x4*>(la) + part : reinterpret_cast<const u32x4*>(la ? la : safe);
      v[i] = u32x4{0u, 0u, 0u, 0u};
    }
    if (used != 0) { // wave-uniform: a wave of out-of-class offsets loads nothing
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = *src[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      tile[r * 8 + (part ^ (r & 7))] = need[i] ? v[i] : u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const u32x4 t = tile[lane * 8 + ((1 + c) ^ (lane & 7))];
      h.d[4 * c + 0] = t.x;
      h.d[4 * c + 1] = t.y;
      h.d[4 * c + 2] = t.z;
      h.d[4 * c + 3] = t.w;
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = tile[lane * 8 + (0 ^ (lane & 7))].w >> 16;
  } else if (use) {
    // Per-lane window: chunk c spans eth + (14 - MIS) + 16c .. +16 and is loaded whole only inside avail (a chunk
    // past it re-reads chunk 0, a line this lane fetches anyway, and is dropped, so the 7 loads are in flight
    // together).  The one chunk avail ends in is read by dwords, those that begin below avail: a datagram may end
    // in it, and an aligned dword lies in the page of its first byte.
    u32x4 v[kWinChunks];
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const bool in = (uint32_t)(14 - MIS + 16 * c + 16) <= a.avail;
      v[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(win) + (in ? c : 0));
    }
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const uint32_t lo = (uint32_t)(14 - MIS + 16 * c); // the chunk's first byte, relative to eth
      if (lo + 16 <= a.avail) {
        h.d[4 * c + 0] = v[c].x;
        h.d[4 * c + 1] = v[c].y;
        h.d[4 * c + 2] = v[c].z;
        h.d[4 * c + 3] = v[c].w;
      } else if (lo < a.avail) { // wave-uniform
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (lo + 4 * q < a.avail) h.d[4 * c + q] = reinterpret_cast<const uint32_t*>(win)[4 * c + q];
      }
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = *reinterpret_cast<const uint32_t*>(win - 4) >> 16; // eth + 10
  }
  const uint32_t s0 = stream_start((uint64_t)win);

  const uint32_t ver_ihl = h.template b8<MIS + 0>();
  const uint32_t tot_len = bswap16(h.template u16<MIS + 2>());
  const uint32_t frag = bswap16(h.template u16<MIS + 6>());
  const uint32_t proto = h.template b8<MIS + 9>();
  const uint32_t src_ip = h.template u32<MIS + 12>();
  const uint32_t dst_ip = h.template u32<MIS + 16>();
  const uint32_t src_port = h.template u16<MIS + 20>();
  const uint32_t dst_port = h.template u16<MIS + 22>();
  const uint32_t ulen_raw = h.template u16<MIS + 24>();
  const uint32_t ulen = bswap16(ulen_raw);
  const uint32_t csum = h.template u16<MIS + 26>();

  uint32_t flags = 0;
  if (ether_type != 0x0008 || (ver_ihl >> 4) != 4 || proto != 17) flags |= PN_UF_NOT_UDP;
  if ((ver_ihl & 0xf) != 5) flags |= PN_UF_IHL_NE_5;
  if (frag & 0x3FFF) flags |= PN_UF_FRAG;
  if (ulen < 8 || tot_len < 28 || ulen > tot_len - 20) flags |= PN_UF_LEN_BAD;
  const uint32_t ulen_even = (ulen + 1) & ~1u;
  if (34 + ulen_even > a.avail) flags |= PN_UF_TRUNC;
  const uint32_t s_ip20 = h.template sum16<MIS, MIS + 20>();
  if (csum_fold(s_ip20) == 0) flags |= PN_UF_IP_OK;

  const bool filter = use && !(flags & (PN_UF_NOT_UDP | PN_UF_IHL_NE_5 | PN_UF_FRAG));
  const uint32_t sub_id = udp_probe(a, dst_ip, dst_port, filter);
  if (sub_id != PN_UDP_NO_SUB) flags |= PN_UF_MATCH;
  const bool checkable = (flags & (PN_UF_MATCH | PN_UF_LEN_BAD | PN_UF_TRUNC)) == PN_UF_MATCH;
  if (checkable && csum == 0) flags |= PN_UF_NOCSUM;
  const bool summed = checkable && csum != 0;
  if (HO && summed) flags |= PN_UF_UDP_UNCHECKED;

  if constexpr (!HO) {
    // ---- phase 2 ----  summed extent relative to the window: [MIS, MIS + 20 + ulen_even); bit 0 flags an odd
    // ulen, whose last summed byte (end - 1) is the byte after the datagram
    const int end_rel = summed ? (int)((MIS + 20 + ulen_even) | (ulen & 1)) : 0;
    uint32_t t_all = window_part<MIS>(h, end_rel & ~1, s0);
    uint32_t pad = kPadUnknown;
    const uint64_t smask = __ballot(end_rel != 0);
    if (smask != 0) { // a wave none of whose frames is summed streams nothing
      const uint32_t e16 = (uint32_t)((end_rel & ~1) + 3) & ~3u;
      const bool short_frame = live && e16 <= s0 + 1024; // a frame that is not summed is one
      constexpr int kFull = kProdAbl & ~(kSkipEmptyLoads | kSkipWaveGate);
      const uint32_t cnt = (uint32_t)__builtin_popcountll(smask);
      if (__ballot(short_frame) == 0) {
        stream_phase<kFull, kLoadAux, 1>(0, nullptr, (uint64_t)win, n_here, lane, end_rel, t_all, pad);
      } else if (cnt == n_here) {
        stream_phase<kProdAbl, kLoadAux, 1>(0, nullptr, (uint64_t)win, n_here, lane, end_rel, t_all, pad);
      } else {
        // few of the wave's frames are summed: compact them onto the first cnt lanes (lane j takes the j-th summed
        // frame's window address and extent, the others go behind), stream those alone, then fetch each frame's
        // total and pad byte back to its own lane -- the strided kernel's mixed-wave form
        const uint32_t rank = (uint32_t)__builtin_popcountll(smask & ((1ull << lane) - 1));
        const int to = (int)(4 * (end_rel != 0 ? rank : cnt + ((uint32_t)lane - rank)));
        const int c_end = __builtin_amdgcn_ds_permute(to, end_rel);
        const uint32_t c_lo = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)(uintptr_t)win);
        const uint32_t c_hi = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)((uintptr_t)win >> 32));
        uint32_t c_t = 0, c_pad = kPadUnknown;
        stream_phase<kProdAbl, kLoadAux, 1>(0, nullptr, ((uint64_t)c_hi << 32) | c_lo, cnt, lane, c_end, c_t, c_pad);
        const uint32_t b_t = (uint32_t)__builtin_amdgcn_ds_bpermute(to, (int)c_t);
        const uint32_t b_pad = (uint32_t)__builtin_amdgcn_ds_bpermute(to, (int)c_pad);
        if (end_rel != 0) {
          t_all += b_t;
          pad = b_pad;
        }
      }
    }
    // ---- phase 3 ----
    if (summed) {
      uint32_t s_seg = t_all - s_ip20; // exact: both are exact word sums
      if (ulen & 1) { // RFC 768 pads with zero: take the byte after the datagram (high half of the last word) out
        uint32_t b = pad;
        if (b == kPadUnknown) b = (win + MIS)[20 + ulen]; // below the stream start, or past its two KiBs
        s_seg -= b << 8;
      }
      const uint32_t s_addr = (src_ip >> 16) + (src_ip & 0xffff) + (dst_ip >> 16) + (dst_ip & 0xffff);
      // pseudo-header: protocol 17 and the UDP length, as words in the order they are stored
      if (csum_fold(s_addr + 0x1100 + ulen_raw + s_seg) == 0) flags |= PN_UF_UDP_OK;
    }
  }

  if (live) {
    u32x4 rec;
    rec.x = sub_id;
    rec.y = src_ip;
    rec.z = src_port | (42u << 16);
    rec.w = ((ulen - 8) & 0xffff) | (flags << 16);
    if (bad_off) rec = u32x4{PN_UDP_NO_SUB, 0u, 0u, PN_UF_BADOFF << 16}; // outside the call's class: not parsed
    // one coalesced store per wave through a wave-uniform descriptor over the 64-record block the wave's
    // frames lie in (they never cross a 64-frame boundary)
    const uint32_t blk = __builtin_amdgcn_readfirstlane(f & ~63u);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc((const uint8_t*)(a.out + blk), 64 * 16);
    __builtin_amdgcn_raw_buffer_store_b128(rec, ro, (f & 63u) * 16, 0, kStoreAux);
  }
}

// ---- host side ----

template <int MIS>
void udp_indexed_launch(const UdpIdxArgs& a, bool verify, hipStream_t s) {
  const dim3 grid((a.n + a.fpw - 1) / a.fpw), block(kWave);
  if (verify) hipLaunchKernelGGL((udp_indexed_kernel<MIS, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((udp_indexed_kernel<MIS, true>), grid, block, 0, s, a);
}

} // namespace
