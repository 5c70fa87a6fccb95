// udp_indexed.hpp — the indexed UDP receive kernel (and its launch helper) behind pn_udp_classify_indexed:
// pn_udp_classify's record for frames that lie wherever an RX event, a packet-mmap block or a packed capture put
// them -- frame i's Ethernet header at base + offsets[i] -- as pn_classify_indexed is to pn_classify.  The ring
// EfviUdpReceiver reads from (Efvi.h:140, 194-200: pkt_bufs + id * PKT_BUF_SIZE + 64 + prefix_len) is classified
// where the NIC wrote it, in event order.
// Included by udp_indexed_kernel.hip only; everything is internal linkage.
//
// Phases 1 and 3 are udp_classify.hpp's, specialised on MIS = (eth_mod16 + 14) % 16.  What differs is phase 1's
// load: lane f loads offsets[f]; an offset outside the launch's class is not parsed (PN_UF_BADOFF) and none of its
// bytes are read; the others get their window from base + offsets[f] + 14 - MIS through the frame pass's indexed
// loader, no byte at or past avail used.  Phase 2 streams by per-frame address, in this kernel's own copy of the
// gate and the compaction; records are in offsets order.
#pragma once

#include "udp_classify.hpp"

namespace {

struct UdpIdxArgs : UdpArgs { // frames = base, avail = the call's; stride and ipa_off are 0
  const uint64_t* offs;
};

template <int MIS, bool HO>
__global__ __launch_bounds__(kWave, 4) void udp_indexed_kernel(UdpIdxArgs a) {
  const int lane = threadIdx.x;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t f = wave_base + lane;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  const bool live = (uint32_t)lane < n_here;

  const uint64_t o = live ? a.offs[f] : 0;
  const bool bad_off = live && ((o + 14) & 15) != (uint64_t)MIS;
  const bool use = live && !bad_off;
  const uint8_t* win = a.frames + o + 14 - MIS; // ip - MIS; dereferenced by `use` lanes only
  Window h;
  const uint32_t ether_type = load_window_indexed<MIS, 1, kIdxWin>(win, o, use, a.avail, lane, h);
  const uint32_t s0 = stream_start((uint64_t)win);
  const UdpFrame fr = udp_header_phase<MIS, HO>(h, ether_type, use, a);
  uint32_t t_all = 0, pad = kPadUnknown;
  if constexpr (!HO) {
    // phase 2 in the order this kernel has had it since it was written, not through udp_stream: the shared form
    // measured 0.4 % slower on the mixed-wave leg.  A change to the gate or the compaction there is
    // made here too.
    const int end_rel = fr.end_rel;
    t_all = window_part<MIS>(h, end_rel & ~1, s0);
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
      } else { // the strided kernel's mixed-wave form
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
  }
  udp_finish<MIS, HO>(a, fr, f, win, t_all, pad, live, bad_off);
}

// ---- host side ----

template <int MIS>
void udp_indexed_launch(const UdpIdxArgs& a, bool verify, hipStream_t s) {
  const dim3 grid((a.n + a.fpw - 1) / a.fpw), block(kWave);
  if (verify) hipLaunchKernelGGL((udp_indexed_kernel<MIS, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((udp_indexed_kernel<MIS, true>), grid, block, 0, s, a);
}

} // namespace
