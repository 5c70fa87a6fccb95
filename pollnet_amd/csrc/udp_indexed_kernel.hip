// pn_udp_classify_indexed: the UDP receive path over frames named by offsets -- an ef_vi RX-event run over the
// packet-buffer ring, a packet-mmap block, a packed capture -- with the subscriptions of pn_udp_set_subs
// (udp_kernel.hip).  The kernel is in udp_indexed.hpp.
#include "udp_indexed.hpp"

namespace {
using pn_internal::hip_err;
using pn_internal::set_err;
} // namespace

extern "C" {

int pn_udp_classify_indexed(pn_ctx* ctx, const void* base, const uint64_t* offsets, uint32_t eth_mod16, uint32_t n,
                            uint32_t avail, void* results, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_classify_indexed: ctx is NULL");
  UdpIdxArgs a;
  if (int rc = udp_common_args(ctx, "pn_udp_classify_indexed", results, n, a)) return rc;
  if (n == 0) return PN_OK;
  if (!base || !offsets || !results) return set_err(ctx, PN_EINVAL, "pn_udp_classify_indexed: NULL buffer");
  if (((uintptr_t)base & 15) || ((uintptr_t)results & 15) || ((uintptr_t)offsets & 7))
    return set_err(ctx, PN_EINVAL, "pn_udp_classify_indexed: base/results must be 16-byte, offsets 8-byte aligned");
  if (eth_mod16 > 15 || (eth_mod16 & 1) || avail < 96 || avail > 65536)
    return set_err(ctx, PN_EINVAL, "pn_udp_classify_indexed: eth_mod16 must be even < 16, avail in [96, 65536]");
  a.frames = (const uint8_t*)base;
  a.stride = 0;
  a.ipa_off = 0;
  a.avail = avail;
  a.offs = offsets;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  const bool verify = ctx->verify_tcp;
  for_mis(eth_mod16, [&](auto mis) { udp_indexed_launch<mis()>(a, verify, s); });
  e = hipGetLastError();
  if (e != hipSuccess) return hip_err(ctx, e, "udp_indexed launch");
  pn_internal::note_stream(ctx, s);
  return PN_OK;
}

} // extern "C"
