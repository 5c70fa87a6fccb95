// tx_fill.hpp — the TX checksum-fill kernels (device code + launch helpers), shared by the
// product library (tx_kernel.hip: pn_tx_fill, pn_tx_fill_notify) and the tuning library
// (tx_tuning.hip: the ablated same-run ceiling).  Internal linkage; one including translation
// unit per library.
#pragma once
// MI355X (gfx950) TX checksum fill for a batch of outgoing frames.
//
// Reference: efvitcp never sums a frame in one pass; it carries one's-complement
// state per connection and per send buffer and folds it when the frame leaves:
//   TcpConn::reset / onEstablished cache the header sums (TcpConn.h:149-186, :422-428),
//   sendPartial adds each appended piece with copyAndSum (TcpConn.h:238-240, :257-299),
//   sendBuf adds seq/ack/window/timestamps (TcpConn.h:310-323),
//   SendBuf::setOptDataLen writes tot_len and folds both sums (Core.h:157-163);
//   resendUna patches the folded sum in place (TcpConn.h:771-785), sumRst builds
//   RST / TIME_WAIT ACKs the same way (Core.h:385-398).  Efvi's UDP sender caches the
//   IPv4 header sum once and folds it with each length (Efvi.h:405-411, 611-621).
// Every one of those sums is congruent (mod 0xFFFF) to the plain RFC 1071 word sum of
// the bytes that end up in the frame and is never 0, so CSum::fold of either gives the
// same 16 bits: the kernel recomputes both checksums from the frame
// bytes in one HBM pass and writes the values the reference's incremental path writes.
// Efvi's cached fold is not CSum::fold: when the first end-around step of the cached
// header sum carries, `cache += cache >> 16` keeps the carry bit and adds it again, so
// the cache is one too large and the header checksum written with it does not verify
// (DESIGN.md §12).  PN_TX_UDP_EFVI reproduces Efvi bit for bit, defect included;
// PN_TX_UDP writes the same fields with CSum::fold (equal to Efvi everywhere else).
//
// Two kernels:
//  tx_fill_kernel   rx_kernel.hip's frame pass (frame_pass.hpp) — one wave per 64
//                   slots, header window per lane, wave-wide 1-KiB streaming of each
//                   frame's segment with exact dot2 word sums — then the field values,
//                   either stored into the frame (2-byte stores) or as one 8-B patch
//                   record per frame, written coalesced to ctx scratch.
//  tx_patch_kernel  one lane per frame writes its 2-byte fields from its patch record.
// A call of up to kTxInPlaceMaxFrames frames is one launch writing in place; a larger one is
// two launches, the fill writing records and the patch kernel the frames.  On 1 Mi frames the
// in-place stores land on partially written lines in the middle of the read stream and cost a
// third of the kernel; as a separate short phase the same stores cost a fifth.  No other
// phase-2 store form measured faster than the 2-byte stores (with every shape
// that was tried under "Retired TX variants").
// HBM-bound: reads tot_len bytes (+ the Ethernet line head), writes 4-8 bytes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/pollnet_amd.h"
#include "device_common.hpp"
#include "frame_pass.hpp"
#include "pn_internal.hpp"

namespace {

using namespace pn_dev;
using pn_internal::hip_err;
using pn_internal::set_err;

struct TArgs {
  uint8_t* frames;
  const uint16_t* lens; // setOptDataLen's len / update_udp_pkt's paylen per frame, or nullptr
  uint32_t n;
  uint32_t stride;
  uint32_t ipa_off;  // (frame_off + 14) & ~15
  uint32_t avail;    // stride - frame_off
  uint32_t frame_off;
  uint2* patch;      // n patch records (ctx scratch)
  uint32_t fpw = kFramesPerWave; // frames per wave (8..64, frames_per_wave)
  uint32_t* sig_count = nullptr;  // SIG (pn_tx_fill_notify): workgroups finished, device memory
  uint32_t* sig_flag = nullptr;   // SIG: host-visible word the last workgroup sets to sig_token
  uint32_t sig_token = 0;
};

// Patch record: x = ip checksum | (tcp checksum or udp_len) << 16, y = tot_len word | flags << 16
constexpr uint32_t kPatchOk = 1u << 16, kPatchLen = 2u << 16;

__device__ __forceinline__ void st16(uint8_t* p, uint32_t v) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)v; }

// Where the field values go.  WB = 0 (calls of up to kTxInPlaceMaxFrames frames): 2-byte stores straight
// into the frame.  WB = kWbPatch (larger calls): the patch record, for tx_patch_kernel.
constexpr int kWbPatch = -2;

// The stream phase's options (SABL).  Every stream load is issued (kExactRange alone, no
// kSkipEmptyLoads): TX batches are mostly full-size frames, where skipping the empty loads measured
// slower.  The window loads go out one round trip apart (kSerialWindow), not all at once as in the RX
// kernel: the fill measured 1.3-2.5 % faster that way.  Phase 2 is not pipelined by half batches: that
// gained 0.1-0.2 % here.  Measurements: DESIGN.md §12.
constexpr int kTxStream = kExactRange | kSerialWindow;

// MIS: the alignment class (frame_off + 14) % 16.  COOP: the cooperative header window (coop_layout).
// MODE: PN_TX_TCP, PN_TX_UDP_EFVI or PN_TX_UDP.  SABL: kTxStream, or with kAblNoReduce for the timing-only
// ceiling (pn_calib_tx_ablated).  SIG: completion word (pn_tx_fill_notify, signal_done in frame_pass.hpp).
// The parameter list is frozen: the demangled kernel names are keys in profiles/pmc_traffic.json.  SAUX, LAUX0
// (cache policies of a line write-back and of the window loads), PADK (LDS padding) and XCD (false: blockIdx
// order) have one live value each, as do WB's other write-back forms and SABL's other bits: they selected
// shapes that were measured and retired ("Retired TX variants").  The line-0 window loads keep the
// default policy (LAUX0 = 0, not nt), so the line the fields are later written to is still cached; workgroups
// take the batch in XCD-contiguous order (xcd_group), as the RX kernel's do.
template <int MIS, int COOP, int MODE, int WB = kWbPatch, int SAUX = 0, int LAUX0 = 0, int PADK = 0, bool XCD = false,
          int SABL = kTxStream, bool SIG = false>
__global__ __launch_bounds__(kWave, 5) void tx_fill_kernel(TArgs a) {
  static_assert((COOP == 0 || COOP == 1) && (MODE == PN_TX_TCP || MODE == PN_TX_UDP_EFVI || MODE == PN_TX_UDP) &&
                    (WB == 0 || WB == kWbPatch) && SAUX == 0 && LAUX0 == 0 && PADK == 0 && XCD &&
                    (SABL == kTxStream || SABL == (kTxStream | kAblNoReduce)),
                "a retired form of a phase");
  const int lane = threadIdx.x;
  const uint32_t wave_base = xcd_group(blockIdx.x, gridDim.x) * a.fpw;
  if (wave_base >= a.n) return;
  const uint32_t f = wave_base + lane;
  const uint32_t n_here = min(a.fpw, a.n - wave_base);
  const bool live = (uint32_t)lane < n_here;
  uint8_t* wave_slot = a.frames + (uint64_t)wave_base * a.stride;
  const __amdgpu_buffer_rsrc_t rs = frame_rsrc(wave_slot, n_here * a.stride);

  Window h;
  (void)load_window_strided<MIS, COOP, LAUX0, (SABL & kSerialWindow) != 0>(rs, lane, a.stride, a.ipa_off,
                                                                           (uint32_t)(uintptr_t)wave_slot, h);
  uint8_t* ip = wave_slot + (uint64_t)lane * a.stride + a.ipa_off + MIS;

  // IpHeader (Core.h:57-69): tot_len at ip+2, checksum at ip+10
  const uint32_t tot_word_old = h.template u16<MIS + 2>();
  const uint32_t ip_chk_old = h.template u16<MIS + 10>();
  uint32_t tot = bswap16(tot_word_old);
  constexpr bool UDP = MODE != PN_TX_TCP;
  constexpr uint32_t kHdr = UDP ? 28 : 40; // ip + udp / ip + tcp without options
  const bool has_len = a.lens != nullptr;
  uint32_t len = 0;
  if (has_len && live) {
    len = a.lens[f];
    tot = (kHdr + len) & 0xffff; // htons(40 + len) (Core.h:158), htons(28 + paylen) (Efvi.h:615)
  }
  const bool ok = live && tot >= kHdr && 14 + tot <= a.avail;
  const uint32_t tot_word = bswap16(tot);
  const uint32_t s_ip_stored = h.template sum16<MIS, MIS + 20>(); // the 20 bytes as they are in memory
  // the header's words with checksum 0 and the new tot_len (exact: both removed words are terms of s_ip_stored)
  const uint32_t s_ip = s_ip_stored - ip_chk_old - tot_word_old + tot_word;

  uint32_t ip_chk, l4; // l4: tcp checksum (TCP) or udp_len word (UDP)
  if constexpr (UDP) {
    if constexpr (MODE == PN_TX_UDP_EFVI) {
      // Efvi: ipsum_cache over the header with tot_len = check = 0 (Efvi.h:405-411), then
      // ipsum = cache + iplen; ipsum += ipsum >> 16; check = ~ipsum & 0xffff (Efvi.h:615-617)
      uint32_t cache = s_ip - tot_word;
      cache = (cache >> 16) + (cache & 0xffff);
      cache += cache >> 16;
      uint32_t ipsum = cache + tot_word;
      ipsum += ipsum >> 16;
      ip_chk = ~ipsum & 0xffff;
    } else {
      ip_chk = csum_fold(s_ip);
    }
    l4 = bswap16((8 + len) & 0xffff); // udp_len = htons(8 + paylen) (Efvi.h:618)
  } else {
    // summed extent [ip, ip + tot) rounded up to a whole word; bit 0 flags an odd tot_len,
    // whose last word holds the byte after the segment (zero-padded in the sum: copyAndSum
    // adds a trailing odd byte as the low byte of a word, TcpConn.h:291-295)
    const uint32_t even_end = MIS + ((tot + 1) & ~1u);
    const int end_rel = ok ? (int)(even_end | (tot & 1)) : 0;
    uint32_t t_all = window_part<MIS>(h, end_rel & ~1, stream_start((uint64_t)(ip - MIS)));
    uint32_t pad = kPadUnknown;
    stream_phase<SABL, kLoadAux, 0>(a.stride, wave_slot + a.ipa_off, 0, n_here, lane, end_rel, t_all, pad);
    if (ok && (tot & 1) && pad == kPadUnknown) pad = ip[tot]; // pad byte inside the window
    const uint32_t tcp_chk_old = h.template u16<MIS + 36>(); // TcpHeader.checksum at tcp+16 (Core.h:84)
    const uint32_t s_seg = t_all - s_ip_stored - tcp_chk_old - ((tot & 1) ? (pad << 8) : 0u);
    const uint32_t src_ip = h.template u32<MIS + 12>(), dst_ip = h.template u32<MIS + 16>();
    const uint32_t s_addr = (src_ip >> 16) + (src_ip & 0xffff) + (dst_ip >> 16) + (dst_ip & 0xffff);
    // pseudo-header: src, dst, ntohs(6), htons(20 + len) (TcpConn.h:165-167, Core.h:160)
    l4 = csum_fold(s_addr + 0x0600 + bswap16(tot - 20) + s_seg);
    ip_chk = csum_fold(s_ip);
  }

  if constexpr (WB == kWbPatch) {
    if (live) {
      const uint2 rec = {ip_chk | (l4 << 16), tot_word | (ok ? kPatchOk : 0u) | (has_len ? kPatchLen : 0u)};
      a.patch[f] = rec; // one coalesced 512-B store per wave
    }
  } else { // in place: tot_len at ip+2, the IP checksum at ip+10, the TCP checksum at ip+36 / udp_len at ip+24
    constexpr int L4 = UDP ? 24 : 36;
    if (ok) {
      if (has_len) st16(ip + 2, tot_word);
      st16(ip + 10, ip_chk);
      if (!UDP || has_len) st16(ip + L4, l4);
    }
  }
  if constexpr (SIG) signal_done(a.sig_count, a.sig_flag, a.sig_token, lane);
}

// Phase 2: one lane per frame writes the fields its patch record carries, with plain 2-byte stores
// (PV = 0; the non-temporal form is retired).  Global stores: a per-lane buffer descriptor
// would be waterfalled.  The parameter list is frozen like tx_fill_kernel's.
template <int MODE, int PV = 0>
__global__ __launch_bounds__(256) void tx_patch_kernel(TArgs a) {
  static_assert(PV == 0, "a retired form of a phase");
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.n) return;
  const uint2 rec = a.patch[f];
  if (!(rec.y & kPatchOk)) return;
  uint8_t* ip = a.frames + (uint64_t)f * a.stride + a.frame_off + 14;
  if (rec.y & kPatchLen) st16(ip + 2, rec.y);
  st16(ip + 10, rec.x);
  if constexpr (MODE == PN_TX_TCP) st16(ip + 36, rec.x >> 16);
  else if (rec.y & kPatchLen) st16(ip + 24, rec.x >> 16);
}

// ---- host side: arguments and launches ----

// The kernel arguments of a batch: n slots of `slot_stride` bytes at `frames`, each frame's Ethernet header
// frame_off into its slot; the patch records go to the ctx's scratch as it is now (ensure_patch first).
inline TArgs tx_args(pn_ctx* ctx, void* frames, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                     const uint16_t* lens) {
  TArgs a;
  a.frames = (uint8_t*)frames;
  a.lens = lens;
  a.n = n;
  a.stride = slot_stride;
  a.ipa_off = (frame_off + 14) & ~15u;
  a.avail = slot_stride - frame_off;
  a.frame_off = frame_off;
  a.patch = (uint2*)ctx->tx_patch;
  a.fpw = frames_per_wave(n);
  return a;
}

inline bool coop_layout(const TArgs& a) {
  return (a.stride % 16) == 0 && a.ipa_off >= 16 && ((uintptr_t)a.frames % 16) == 0;
}

// Up to this many frames a call is ONE launch writing the fields in place: the batch's lines
// are still cached when they are written, and the patch launch's ≈2-µs boundary is the larger
// cost (1.5-4.6 µs less per call from 16 to 65,536 frames, pinned host or device memory,
// profiles/r02/tx_fill_small_batches.json).  Above it the two phases (the in-place
// writes' write-back would land in the rest of the stream).
constexpr uint32_t kTxInPlaceMaxFrames = 65536;

// f(std::integral_constant<int, MODE>{}) for a valid pn_tx_fill mode, as for_mis for the alignment class.
template <class F>
void for_tx_mode(uint32_t mode, F&& f) {
  switch (mode) {
    case PN_TX_TCP: return f(std::integral_constant<int, PN_TX_TCP>{});
    case PN_TX_UDP_EFVI: return f(std::integral_constant<int, PN_TX_UDP_EFVI>{});
    default: return f(std::integral_constant<int, PN_TX_UDP>{});
  }
}

// One fill launch of the batch's alignment class, with the cooperative window where the layout allows.
template <int MODE, int WB, bool SIG = false>
void launch(const TArgs& a, hipStream_t s) {
  const dim3 grid((a.n + a.fpw - 1) / a.fpw), block(kWave);
  for_mis(a.frame_off, [&](auto mis) {
    if (coop_layout(a)) {
      hipLaunchKernelGGL((tx_fill_kernel<mis(), 1, MODE, WB, 0, 0, 0, true, kTxStream, SIG>), grid, block, 0, s, a);
      return;
    }
    hipLaunchKernelGGL((tx_fill_kernel<mis(), 0, MODE, WB, 0, 0, 0, true, kTxStream, SIG>), grid, block, 0, s, a);
  });
}

// pn_tx_fill's launches: in place up to kTxInPlaceMaxFrames, the two phases above.
template <int MODE>
void launch_mode(const TArgs& a, hipStream_t s) {
  if (a.n <= kTxInPlaceMaxFrames) {
    launch<MODE, 0>(a, s);
    return;
  }
  launch<MODE, kWbPatch>(a, s);
  hipLaunchKernelGGL((tx_patch_kernel<MODE>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

inline int check_args(pn_ctx* ctx, void* frames, uint32_t slot_stride, uint32_t frame_off, const uint16_t* lens) {
  if (!frames) return set_err(ctx, PN_EINVAL, "pn_tx_fill: NULL frames");
  if (((uintptr_t)frames & 15) || ((uintptr_t)lens & 1))
    return set_err(ctx, PN_EINVAL, "pn_tx_fill: frames must be 16-byte, lens 2-byte aligned");
  if ((slot_stride & 15) || slot_stride > 65536 || (frame_off & 1) || slot_stride < frame_off + 96)
    return set_err(ctx, PN_EINVAL, "pn_tx_fill: slot_stride/frame_off violate the layout contract");
  return PN_OK;
}

// ctx-owned patch scratch, grown on demand.  A call on another stream than the previous
// scratch user is ordered after it on the device (pn_fence: no per-launch event, no host wait);
// growing it waits on the host for that user before the old scratch is freed.
inline int ensure_patch(pn_ctx* ctx, uint32_t n, hipStream_t s) {
  if (n > ctx->tx_patch_n) {
    if (ctx->tx_patch) {
      const int rc = pn_internal::fence_host_wait(ctx, ctx->tx);
      if (rc) return rc;
      (void)hipFree(ctx->tx_patch);
      ctx->tx_patch = nullptr;
      ctx->tx_patch_n = 0;
    }
    const uint32_t cap = n < (1u << 16) ? (1u << 16) : n;
    hipError_t e = hipMalloc(&ctx->tx_patch, (size_t)cap * sizeof(uint2));
    if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(tx patch scratch)");
    ctx->tx_patch_n = cap;
  }
  return pn_internal::fence_use(ctx, ctx->tx, s);
}

} // namespace
