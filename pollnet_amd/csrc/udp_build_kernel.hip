// pn_udp_set_channels / pn_udp_build: the UDP send path -- wire-ready datagrams built in the slots of a TX ring from
// per-destination header templates (EfviUdpSender's side of pollnet, Efvi.h:339-650).  The kernel is in
// udp_build.hpp.
#include "udp_build.hpp"

#include <cstring>
#include <vector>

namespace {
using pn_internal::hip_err;
using pn_internal::set_err;
} // namespace

extern "C" {

int pn_udp_set_channels(pn_ctx* ctx, const pn_udp_channel* chans, uint32_t n_chans) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_set_channels: ctx is NULL");
  if (n_chans == 0 || n_chans > PN_UDP_MAX_CHANNELS)
    return set_err(ctx, PN_EINVAL, "pn_udp_set_channels: n_chans must be in [1, PN_UDP_MAX_CHANNELS]");
  if (!chans) return set_err(ctx, PN_EINVAL, "pn_udp_set_channels: chans is NULL");
  // checked and built on the host before anything is waited for
  std::vector<uint32_t> tbl((size_t)n_chans * kUbEntryDw, 0);
  for (uint32_t i = 0; i < n_chans; ++i) {
    const uint8_t* h = chans[i].hdr;
    for (uint8_t p : chans[i]._pad)
      if (p) return set_err(ctx, PN_EINVAL, "pn_udp_set_channels: non-zero _pad in channel " + std::to_string(i));
    if (h[12] != 0x08 || h[13] != 0x00 || h[14] != 0x45 || h[23] != 17)
      return set_err(ctx, PN_EINVAL, "pn_udp_set_channels: channel " + std::to_string(i) + " is not IPv4/UDP with IHL 5");
    uint8_t e[4 * kUbEntryDw] = {0};
    memcpy(e, h, kUbHdr);
    e[16] = e[17] = 0; // tot_len
    e[24] = e[25] = 0; // ip checksum
    e[38] = e[39] = 0; // udp_len
    e[40] = e[41] = 0; // udp checksum
    auto w16 = [&](int o) { return (uint32_t)e[o] | ((uint32_t)e[o + 1] << 8); }; // as a little-endian load gives it
    uint32_t cache = 0; // Efvi.h:406-410
    for (int k = 0; k < 10; ++k) cache += w16(14 + 2 * k);
    cache = (cache >> 16) + (cache & 0xffff);
    uint32_t pseudo = 0x1100; // {0, 17} as stored
    for (int o = 26; o < 38; o += 2) pseudo += w16(o); // src, dst, both ports
    while (pseudo >> 16) pseudo = (pseudo >> 16) + (pseudo & 0xffff);
    e[42] = (uint8_t)pseudo;
    e[43] = (uint8_t)(pseudo >> 8);
    memcpy(e + 44, &cache, 4);
    memcpy(&tbl[(size_t)i * kUbEntryDw], e, sizeof(e));
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  // control plane: the one device table is replaced in place, so every launch that may read it finishes first
  int rc = pn_sync(ctx);
  if (rc) return rc;
  if (n_chans > ctx->ub_cap) {
    if (ctx->ub_tbl) (void)hipFree(ctx->ub_tbl);
    ctx->ub_tbl = nullptr;
    ctx->ub_cap = 0;
    ctx->ub_n = 0;
    e = hipMalloc(&ctx->ub_tbl, (size_t)n_chans * kUbEntryDw * sizeof(uint32_t));
    if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(udp channel table)");
    ctx->ub_cap = n_chans;
  }
  if (!ctx->copy_stream) {
    e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_err(ctx, e, "hipStreamCreate(table uploads)");
  }
  e = hipMemcpyAsync(ctx->ub_tbl, tbl.data(), tbl.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
  if (e != hipSuccess) {
    ctx->ub_n = 0; // the table's contents are unknown: no launch until a set succeeds
    return hip_err(ctx, e, "hipMemcpyAsync(udp channel table)");
  }
  ctx->ub_n = n_chans;
  return PN_OK;
}

int pn_udp_build(pn_ctx* ctx, const void* payloads, uint64_t payload_bytes, const uint64_t* pay_offs,
                 const uint16_t* pay_lens, const uint32_t* chan_ids, void* frames, uint32_t slot_stride,
                 uint32_t frame_off, uint32_t n, uint32_t mode, uint16_t* frame_lens, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_build: ctx is NULL");
  if (!ctx->ub_tbl || ctx->ub_n == 0)
    return set_err(ctx, PN_ENOTABLE, "pn_udp_build: no channels (call pn_udp_set_channels)");
  if (n == 0) return PN_OK;
  if (mode != PN_UB_EFVI && mode != PN_UB_PLAIN && mode != PN_UB_CSUM)
    return set_err(ctx, PN_EINVAL, "pn_udp_build: unknown mode");
  if (!payloads || !pay_offs || !pay_lens || !frames || !frame_lens)
    return set_err(ctx, PN_EINVAL, "pn_udp_build: NULL buffer");
  if (((uintptr_t)payloads & 15) || ((uintptr_t)frames & 15) || ((uintptr_t)pay_offs & 7) || ((uintptr_t)pay_lens & 1) ||
      ((uintptr_t)chan_ids & 3) || ((uintptr_t)frame_lens & 1))
    return set_err(ctx, PN_EINVAL,
                   "pn_udp_build: payloads/frames must be 16-byte aligned, the index arrays aligned to their element");
  if ((slot_stride & 15) || slot_stride > 65536 || (frame_off & 1) || slot_stride < frame_off + 96)
    return set_err(ctx, PN_EINVAL, "pn_udp_build: slot_stride/frame_off violate the layout contract");
  UbArgs a;
  a.pay = (const uint8_t*)payloads;
  a.pay_bytes = payload_bytes;
  a.offs = pay_offs;
  a.lens = pay_lens;
  a.chans = chan_ids;
  a.frames = (uint8_t*)frames;
  a.frame_lens = frame_lens;
  a.tbl = ctx->ub_tbl;
  a.n_chans = ctx->ub_n;
  a.n = n;
  a.stride = slot_stride;
  a.frame_off = frame_off;
  a.fpw = frames_per_wave(n);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  ub_launch(a, mode, s);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "udp_build launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

} // extern "C"
