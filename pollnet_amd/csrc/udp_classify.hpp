// udp_classify.hpp — the UDP receive path's device code: the subscription table and its probe, the receive body
// both kernels are made of (udp_header_phase, udp_finish), the strided phase 2 (udp_stream), and the strided kernel
// with its launch helper behind pn_udp_classify.  The indexed kernel is in udp_indexed.hpp.
// It is the NIC filter of EfviUdpReceiver (ef_filter_spec_set_ip4_local(IPPROTO_UDP, ip, port), Efvi.h:143-156) for
// thousands of subscriptions at once, the fields EfviUdpReceiver::read / recvfrom take from fixed offsets
// (Efvi.h:199, 252-253), and the IPv4 / RFC 768 checksum verdicts a NIC gives with EF_EVENT_TYPE_RX.
// Included by udp_kernel.hip and udp_indexed.hpp (one translation unit each); everything is internal linkage.
//
// Same execution model as the RX classify kernel (rx_classify.hpp), built from the same frame pass
// (frame_pass.hpp): one wave per frames_per_wave(n) frames, one-wave workgroups in XCD order, specialised on
// MIS = (frame_off + 14) % 16.
//  phase 1  lane f decodes frame f's header window (IPv4 + UDP header at ip + 20 .. ip + 28) and looks
//           (dst_ip, dst_port) up in the subscription hash table (open addressing, 8-B entries, L2-resident).
//  phase 2  the wave streams [ip, ip + 20 + ulen_even) of the frames that matched, carry a checksum and are being
//           verified -- and of no other frame: a frame for somebody else, or one sent with checksum 0 (Efvi's own
//           sender), costs its header line only.  A wave with only some frames to sum compacts them onto its first
//           lanes and streams those alone (leg (c) -49 %).
//  phase 3  lane f takes the IP header words and the pad byte out, adds the pseudo-header, folds; one coalesced
//           16-B record per lane.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/pollnet_amd.h"
#include "device_common.hpp"
#include "frame_pass.hpp"
#include "pn_internal.hpp"

namespace {

using namespace pn_dev;

struct UdpArgs {
  const uint8_t* frames;
  pn_udp_result* out;
  const uint64_t* tbl; // subscription table: dst_ip | dst_port << 32 | (sub_id + 1) << 48, 0 = empty
  uint32_t tbl_mask;   // capacity - 1 (capacity a power of two >= 2 * n_subs)
  uint32_t n;
  uint32_t stride;
  uint32_t ipa_off; // (frame_off + 14) & ~15: 16-B aligned start of the header window
  uint32_t avail;   // stride - frame_off
  uint32_t fpw;     // frames per wave (frames_per_wave)
};

// The "no subscriptions" check (`fn` names the entry point in its error), then the arguments every UDP receive launch
// takes from the context and the call's records and count, copied as given: the caller still validates n, the
// buffers and the layout before it launches.
inline int udp_common_args(pn_ctx* ctx, const char* fn, void* results, uint32_t n, UdpArgs& a) {
  if (!ctx->udp_tbl || ctx->udp_n == 0)
    return pn_internal::set_err(ctx, PN_ENOTABLE, std::string(fn) + ": no subscriptions (call pn_udp_set_subs)");
  a.out = (pn_udp_result*)results;
  a.tbl = ctx->udp_tbl;
  a.tbl_mask = ctx->udp_mask;
  a.n = n;
  a.fpw = frames_per_wave(n);
  return PN_OK;
}

// Home slot of (dst_ip, dst_port), both as stored in the frame; the host builds the table with the same function.
// Subscription sets are typically runs of consecutive ports or groups: the mix spreads those.
__host__ __device__ inline uint32_t udp_sub_hash(uint32_t ip, uint32_t port) {
  uint32_t x = ip ^ (port * 0x9E3779B1u);
  x *= 0x85EBCA6Bu;
  x ^= x >> 15;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// Linear probe from the home slot: one 8-B load per step through a plain per-lane pointer (no descriptor built from
// per-lane values, so no waterfall loop), bounded by the capacity.  At load <= 1/2 almost every lookup ends at its
// first entry.
__device__ __forceinline__ uint32_t udp_probe(const UdpArgs& a, uint32_t dst_ip, uint32_t dst_port, bool want) {
  uint32_t id = PN_UDP_NO_SUB;
  if (want) {
    const uint64_t key = (uint64_t)dst_ip | ((uint64_t)dst_port << 32);
    uint32_t e = udp_sub_hash(dst_ip, dst_port) & a.tbl_mask;
    for (uint32_t step = 0; step <= a.tbl_mask; ++step) {
      const uint64_t ent = a.tbl[e];
      if (ent == 0) break;
      if ((ent & 0xFFFFFFFFFFFFull) == key) {
        id = (uint32_t)(ent >> 48) - 1;
        break;
      }
      e = (e + 1) & a.tbl_mask;
    }
  }
  return id;
}

// Per-frame state the header lane keeps from phase 1 to phase 3.
struct UdpFrame {
  uint32_t flags, sub_id, src_ip, dst_ip, src_port, ulen, ulen_raw, s_ip20;
  // summed extent relative to the window: [MIS, MIS + 20 + ulen_even); bit 0 flags an odd ulen, whose last summed
  // byte (end - 1) is the byte after the datagram.  0: the frame is not summed
  int end_rel;
};

// ---- phase 1: decode one frame from its header window and look its destination up (lane f <-> frame f) ----
// HO: the header-only instantiation (pn_set_verify(ctx, 0)): nothing is summed, PN_UF_UDP_UNCHECKED where a sum was
// due.  `use`: the lane has a frame that is parsed.  The window comes by value on purpose, as the frame state does
// to udp_finish.
template <int MIS, bool HO>
__device__ __forceinline__ UdpFrame udp_header_phase(const Window h, uint32_t ether_type, bool use, const UdpArgs& a) {
  static_assert(MIS + 28 <= kWinBytes, "window must cover ip .. ip+28");
  UdpFrame fr;
  const uint32_t ver_ihl = h.template b8<MIS + 0>();
  const uint32_t tot_len = bswap16(h.template u16<MIS + 2>());
  const uint32_t frag = bswap16(h.template u16<MIS + 6>());
  const uint32_t proto = h.template b8<MIS + 9>();
  fr.src_ip = h.template u32<MIS + 12>();
  fr.dst_ip = h.template u32<MIS + 16>();
  fr.src_port = h.template u16<MIS + 20>();
  const uint32_t dst_port = h.template u16<MIS + 22>();
  fr.ulen_raw = h.template u16<MIS + 24>();
  fr.ulen = bswap16(fr.ulen_raw);
  const uint32_t csum = h.template u16<MIS + 26>();

  uint32_t flags = 0;
  if (ether_type != 0x0008 || (ver_ihl >> 4) != 4 || proto != 17) flags |= PN_UF_NOT_UDP;
  if ((ver_ihl & 0xf) != 5) flags |= PN_UF_IHL_NE_5;
  if (frag & 0x3FFF) flags |= PN_UF_FRAG;
  if (fr.ulen < 8 || tot_len < 28 || fr.ulen > tot_len - 20) flags |= PN_UF_LEN_BAD;
  const uint32_t ulen_even = (fr.ulen + 1) & ~1u;
  if (34 + ulen_even > a.avail) flags |= PN_UF_TRUNC;
  fr.s_ip20 = h.template sum16<MIS, MIS + 20>();
  if (csum_fold(fr.s_ip20) == 0) flags |= PN_UF_IP_OK;

  const bool filter = use && !(flags & (PN_UF_NOT_UDP | PN_UF_IHL_NE_5 | PN_UF_FRAG));
  fr.sub_id = udp_probe(a, fr.dst_ip, dst_port, filter);
  if (fr.sub_id != PN_UDP_NO_SUB) flags |= PN_UF_MATCH;
  const bool checkable = (flags & (PN_UF_MATCH | PN_UF_LEN_BAD | PN_UF_TRUNC)) == PN_UF_MATCH;
  if (checkable && csum == 0) flags |= PN_UF_NOCSUM;
  const bool summed = checkable && csum != 0;
  if (HO && summed) flags |= PN_UF_UDP_UNCHECKED;
  fr.end_rel = (!HO && summed) ? (int)((MIS + 20 + ulen_even) | (fr.ulen & 1)) : 0;
  fr.flags = flags;
  return fr;
}

// ---- phase 2: the wave streams its summed frames, and no other ----
// Strided: frame fi's window at group_ipa + fi * stride, this lane's at `win` (the indexed kernel keeps its own
// copy of this phase, udp_indexed.hpp).  s0 = stream_start(win); t_all comes in holding the window's share (window_part) and leaves with the frame's total,
// pad with the byte after an odd datagram where the stream met it.  Every lane of the wave must call it.
__device__ __forceinline__ void udp_stream(uint32_t stride, const uint8_t* group_ipa, const uint8_t* win, uint32_t s0,
                                           uint32_t n_here, bool live, int lane, int end_rel, uint32_t& t_all,
                                           uint32_t& pad) {
  const uint64_t smask = __ballot(end_rel != 0);
  if (smask == 0) return; // a wave none of whose frames is summed streams nothing
  // the TCP kernel's wave gate: a wave with a frame ending before its second stream KiB (or not streamed at
  // all) takes the skipping form, a wave of full-size frames the form that issues every load
  const uint32_t e16 = (uint32_t)((end_rel & ~1) + 3) & ~3u;
  const bool short_frame = live && e16 <= s0 + 1024;
  constexpr int kFull = kProdAbl & ~(kSkipEmptyLoads | kSkipWaveGate);
  const uint32_t cnt = (uint32_t)__builtin_popcountll(smask);
  if (__ballot(short_frame) == 0) {
    if (stride <= 2048) // no frame reaches past its two stream KiBs: kPipeStream
      return stream_phase_pipelined<kFull, kLoadAux, 0>(stride, group_ipa, (uint64_t)win, n_here, lane, end_rel, t_all, pad);
    return stream_phase<kFull, kLoadAux, 0>(stride, group_ipa, (uint64_t)win, n_here, lane, end_rel, t_all, pad);
  }
  if (cnt == n_here) // every frame is summed: the skipping form over the wave as it lies
    return stream_phase<kProdAbl, kLoadAux, 0>(stride, group_ipa, (uint64_t)win, n_here, lane, end_rel, t_all, pad);
  // A mixed ring: few of the wave's frames are summed.  Compact them onto the first cnt lanes (lane j takes the
  // j-th summed frame's window address and extent; the others go behind, a permutation of the wave) and
  // stream those alone through the frame pass's per-frame-address form, then fetch each frame's total and
  // pad byte back to its own lane: ceil(cnt / 8) batches instead of 8.
  const uint32_t rank = (uint32_t)__builtin_popcountll(smask & ((1ull << lane) - 1));
  const int to = (int)(4 * (end_rel != 0 ? rank : cnt + ((uint32_t)lane - rank)));
  const int c_end = __builtin_amdgcn_ds_permute(to, end_rel);
  const uint32_t c_lo = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)(uintptr_t)win);
  const uint32_t c_hi = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)((uintptr_t)win >> 32));
  uint32_t c_t = 0, c_pad = kPadUnknown;
  stream_phase<kProdAbl, kLoadAux, 1>(stride, group_ipa, ((uint64_t)c_hi << 32) | c_lo, cnt, lane, c_end, c_t, c_pad);
  const uint32_t b_t = (uint32_t)__builtin_amdgcn_ds_bpermute(to, (int)c_t);
  const uint32_t b_pad = (uint32_t)__builtin_amdgcn_ds_bpermute(to, (int)c_pad);
  if (end_rel != 0) {
    t_all += b_t;
    pad = b_pad;
  }
}

// ---- phase 3: fold and write the record on the frame's lane ----
// bad_off (indexed launches): the frame's offset is outside the call's class; it was not parsed.
template <int MIS, bool HO>
__device__ __forceinline__ void udp_finish(const UdpArgs& a, UdpFrame fr, uint32_t f, const uint8_t* win,
                                           uint32_t t_all, uint32_t pad, bool live, bool bad_off) {
  uint32_t flags = fr.flags;
  if (!HO && fr.end_rel != 0) {
    uint32_t s_seg = t_all - fr.s_ip20; // exact: both are exact word sums
    if (fr.ulen & 1) { // RFC 768 pads with zero: take the byte after the datagram (high half of the last word) out
      uint32_t b = pad;
      if (b == kPadUnknown) b = (win + MIS)[20 + fr.ulen]; // below the stream start, or past its two KiBs
      s_seg -= b << 8;
    }
    const uint32_t s_addr = (fr.src_ip >> 16) + (fr.src_ip & 0xffff) + (fr.dst_ip >> 16) + (fr.dst_ip & 0xffff);
    // pseudo-header: protocol 17 and the UDP length, as words in the order they are stored
    if (csum_fold(s_addr + 0x1100 + fr.ulen_raw + s_seg) == 0) flags |= PN_UF_UDP_OK;
  }
  if (live) {
    u32x4 rec;
    rec.x = fr.sub_id;
    rec.y = fr.src_ip;
    rec.z = fr.src_port | (42u << 16);
    rec.w = ((fr.ulen - 8) & 0xffff) | (flags << 16);
    if (bad_off) rec = u32x4{PN_UDP_NO_SUB, 0u, 0u, PN_UF_BADOFF << 16};
    // one coalesced store per wave through a wave-uniform descriptor over the 64-record block the wave's
    // frames lie in (they never cross a 64-frame boundary)
    const uint32_t blk = __builtin_amdgcn_readfirstlane(f & ~63u);
    const __amdgpu_buffer_rsrc_t ro = frame_rsrc((const uint8_t*)(a.out + blk), 64 * 16);
    __builtin_amdgcn_raw_buffer_store_b128(rec, ro, (f & 63u) * 16, 0, kStoreAux);
  }
}

// COOP as load_window_strided's.
template <int MIS, int COOP, bool HO>
__global__ __launch_bounds__(kWave, 4) void udp_classify_kernel(UdpArgs a) {
  const int lane = threadIdx.x;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t f = wave_base + lane;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  const bool live = (uint32_t)lane < n_here;
  const uint8_t* wave_slot = a.frames + (uint64_t)wave_base * a.stride;
  // one wave-uniform descriptor over the wave's slots; lanes past n read zeros
  const __amdgpu_buffer_rsrc_t rs = frame_rsrc(wave_slot, n_here * a.stride);

  Window h;
  const uint32_t ether_type =
      load_window_strided<MIS, COOP, kLoadAux>(rs, lane, a.stride, a.ipa_off, (uint32_t)(uintptr_t)wave_slot, h);
  const uint8_t* win = wave_slot + (uint64_t)lane * a.stride + a.ipa_off; // ip - MIS
  const uint32_t s0 = stream_start((uint64_t)win);
  const UdpFrame fr = udp_header_phase<MIS, HO>(h, ether_type, live, a);
  uint32_t t_all = 0, pad = kPadUnknown;
  if constexpr (!HO) {
    t_all = window_part<MIS>(h, fr.end_rel & ~1, s0);
    udp_stream(a.stride, wave_slot + a.ipa_off, win, s0, n_here, live, lane, fr.end_rel, t_all, pad);
  }
  udp_finish<MIS, HO>(a, fr, f, win, t_all, pad, live, false);
}

// ---- host side ----

// Whether the cooperative header-window load applies (as the RX kernel's coop_layout): a 16-B chunk precedes the
// window inside the slot (frame_off >= 2).  Stride and base are 16-B aligned by the layout contract.
inline bool udp_coop_layout(const UdpArgs& a) { return a.ipa_off >= 16; }

template <int MIS>
void udp_launch(const UdpArgs& a, bool verify, hipStream_t s) {
  const dim3 grid((a.n + a.fpw - 1) / a.fpw), block(kWave);
  if (udp_coop_layout(a)) {
    if (verify) hipLaunchKernelGGL((udp_classify_kernel<MIS, 1, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((udp_classify_kernel<MIS, 1, true>), grid, block, 0, s, a);
  } else if constexpr (MIS == 14) { // frame_off = 0, the one layout with no chunk before the window
    if (verify) hipLaunchKernelGGL((udp_classify_kernel<MIS, 0, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((udp_classify_kernel<MIS, 0, true>), grid, block, 0, s, a);
  }
}

} // namespace
