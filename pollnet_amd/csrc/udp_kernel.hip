// pn_udp_set_subs / pn_udp_classify: the UDP receive path -- subscription demux and checksum verdicts for a batch
// of ring slots (EfviUdpReceiver / SocketUdpReceiver's side of pollnet, Efvi.h:132-273).  The kernel is in
// udp_classify.hpp.
#include "udp_classify.hpp"

#include <vector>

namespace {
using pn_internal::hip_err;
using pn_internal::set_err;
} // namespace

extern "C" {

int pn_udp_set_subs(pn_ctx* ctx, const pn_udp_sub* subs, uint32_t n_subs) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_set_subs: ctx is NULL");
  if (n_subs == 0 || n_subs > PN_UDP_MAX_SUBS)
    return set_err(ctx, PN_EINVAL, "pn_udp_set_subs: n_subs must be in [1, PN_UDP_MAX_SUBS]");
  if (!subs) return set_err(ctx, PN_EINVAL, "pn_udp_set_subs: subs is NULL");
  // open addressing at load <= 1/2, checked and built on the host before anything is waited for
  uint32_t cap = 64;
  while (cap < 2 * n_subs) cap <<= 1;
  std::vector<uint64_t> tbl(cap, 0);
  for (uint32_t i = 0; i < n_subs; ++i) {
    if (subs[i]._pad != 0) return set_err(ctx, PN_EINVAL, "pn_udp_set_subs: non-zero _pad in subscription " + std::to_string(i));
    const uint64_t key = (uint64_t)subs[i].dst_ip | ((uint64_t)subs[i].dst_port << 32);
    uint32_t e = udp_sub_hash(subs[i].dst_ip, subs[i].dst_port) & (cap - 1);
    while (tbl[e] != 0) {
      if ((tbl[e] & 0xFFFFFFFFFFFFull) == key)
        return set_err(ctx, PN_EINVAL, "pn_udp_set_subs: duplicate subscription " + std::to_string(i) + " (same ip and port as " +
                                           std::to_string((uint32_t)(tbl[e] >> 48) - 1) + ")");
      e = (e + 1) & (cap - 1);
    }
    tbl[e] = key | ((uint64_t)(i + 1) << 48);
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  // control plane: the one device table is replaced in place, so every launch that may read it finishes first
  int rc = pn_sync(ctx);
  if (rc) return rc;
  if (cap > ctx->udp_cap) {
    if (ctx->udp_tbl) (void)hipFree(ctx->udp_tbl);
    ctx->udp_tbl = nullptr;
    ctx->udp_cap = 0;
    ctx->udp_mask = 0;
    e = hipMalloc(&ctx->udp_tbl, (size_t)cap * sizeof(uint64_t));
    if (e != hipSuccess) return hip_err(ctx, e, "hipMalloc(udp subscription table)");
    ctx->udp_cap = cap;
  }
  if (!ctx->copy_stream) {
    e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_err(ctx, e, "hipStreamCreate(table uploads)");
  }
  e = hipMemcpyAsync(ctx->udp_tbl, tbl.data(), (size_t)cap * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
  if (e != hipSuccess) {
    ctx->udp_mask = 0;
    ctx->udp_n = 0; // the table's contents are unknown: no launch until a set succeeds
    return hip_err(ctx, e, "hipMemcpyAsync(udp subscription table)");
  }
  ctx->udp_mask = cap - 1;
  ctx->udp_n = n_subs;
  return PN_OK;
}

int pn_udp_classify(pn_ctx* ctx, const void* frames, uint32_t slot_stride, uint32_t frame_off, uint32_t n, void* results,
                    void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_classify: ctx is NULL");
  UdpArgs a;
  if (int rc = udp_common_args(ctx, "pn_udp_classify", results, n, a)) return rc;
  if (n == 0) return PN_OK;
  if (!frames || !results) return set_err(ctx, PN_EINVAL, "pn_udp_classify: NULL buffer");
  if (((uintptr_t)frames & 15) || ((uintptr_t)results & 15))
    return set_err(ctx, PN_EINVAL, "pn_udp_classify: frames/results must be 16-byte aligned");
  if ((slot_stride & 15) || slot_stride > 65536 || (frame_off & 1) || slot_stride < frame_off + 96)
    return set_err(ctx, PN_EINVAL, "pn_udp_classify: slot_stride/frame_off violate the layout contract");
  a.frames = (const uint8_t*)frames;
  a.stride = slot_stride;
  a.ipa_off = (frame_off + 14) & ~15u;
  a.avail = slot_stride - frame_off;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  const bool verify = ctx->verify_tcp;
  for_mis(frame_off, [&](auto mis) { udp_launch<mis()>(a, verify, s); });
  e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "udp_classify launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

} // extern "C"
