// pn_udp_gather / pn_udp_gather_indexed: the UDP gather path -- the delivered payloads of a classified ring packed
// in arrival order into one buffer, with index arrays in pn_udp_build's input format.  The kernels are in
// udp_gather.hpp.
#include "udp_gather.hpp"

namespace {
using pn_internal::hip_err;
using pn_internal::set_err;

// The checks both entry points share: the outputs and the records.  `total` first: n == 0 needs nothing else.
int ug_check_outputs(pn_ctx* ctx, const char* who, uint32_t n, const void* results, void* payloads,
                     uint64_t payload_cap, uint64_t* pay_offs, uint16_t* pay_lens, uint32_t* sub_ids,
                     uint32_t* src_index, pn_udp_gather_total* total) {
  const std::string w(who);
  if (!total) return set_err(ctx, PN_EINVAL, w + ": NULL total");
  if ((uintptr_t)total & 7) return set_err(ctx, PN_EINVAL, w + ": total must be 8-byte aligned");
  if (n == 0) return PN_OK;
  if (!results || !payloads || !pay_offs || !pay_lens || !sub_ids) return set_err(ctx, PN_EINVAL, w + ": NULL buffer");
  if (((uintptr_t)results & 15) || ((uintptr_t)payloads & 15) || (payload_cap & 15) || ((uintptr_t)pay_offs & 7) ||
      ((uintptr_t)pay_lens & 1) || ((uintptr_t)sub_ids & 3) || ((uintptr_t)src_index & 3))
    return set_err(ctx, PN_EINVAL,
                   w + ": results/payloads must be 16-byte aligned, payload_cap a multiple of 16, the index arrays "
                       "aligned to their element");
  return PN_OK;
}

void ug_fill(UgArgs& a, const void* results, void* payloads, uint64_t payload_cap, uint64_t* pay_offs,
             uint16_t* pay_lens, uint32_t* sub_ids, uint32_t* src_index, pn_udp_gather_total* total, uint32_t n) {
  a.results = (const u32x4*)results;
  a.pay = (uint8_t*)payloads;
  a.cap = payload_cap;
  a.pay_offs = pay_offs;
  a.pay_lens = pay_lens;
  a.sub_ids = sub_ids;
  a.src_index = src_index;
  a.total = total;
  a.n = n;
}
} // namespace

extern "C" {

int pn_udp_gather(pn_ctx* ctx, const void* frames, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                  const void* results, void* payloads, uint64_t payload_cap, uint64_t* pay_offs, uint16_t* pay_lens,
                  uint32_t* sub_ids, uint32_t* src_index, pn_udp_gather_total* total, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_gather: ctx is NULL");
  if (int rc = ug_check_outputs(ctx, "pn_udp_gather", n, results, payloads, payload_cap, pay_offs, pay_lens, sub_ids,
                                src_index, total))
    return rc;
  UgArgs a = {};
  if (n) {
    if (!frames) return set_err(ctx, PN_EINVAL, "pn_udp_gather: NULL buffer");
    if ((uintptr_t)frames & 15) return set_err(ctx, PN_EINVAL, "pn_udp_gather: frames must be 16-byte aligned");
    if ((slot_stride & 15) || slot_stride > 65536 || (frame_off & 1) || slot_stride < frame_off + 96)
      return set_err(ctx, PN_EINVAL, "pn_udp_gather: slot_stride/frame_off violate the layout contract");
    a.frames = (const uint8_t*)frames;
    a.offs = nullptr;
    a.stride = slot_stride;
    a.frame_off = frame_off;
    a.avail = slot_stride - frame_off;
  }
  ug_fill(a, results, payloads, payload_cap, pay_offs, pay_lens, sub_ids, src_index, total, n);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  return ug_launch(ctx, a, (hipStream_t)stream);
}

int pn_udp_gather_indexed(pn_ctx* ctx, const void* base, const uint64_t* offsets, uint32_t eth_mod16, uint32_t n,
                          uint32_t avail, const void* results, void* payloads, uint64_t payload_cap,
                          uint64_t* pay_offs, uint16_t* pay_lens, uint32_t* sub_ids, uint32_t* src_index,
                          pn_udp_gather_total* total, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_gather_indexed: ctx is NULL");
  if (int rc = ug_check_outputs(ctx, "pn_udp_gather_indexed", n, results, payloads, payload_cap, pay_offs, pay_lens,
                                sub_ids, src_index, total))
    return rc;
  UgArgs a = {};
  if (n) {
    if (!base || !offsets) return set_err(ctx, PN_EINVAL, "pn_udp_gather_indexed: NULL buffer");
    if (((uintptr_t)base & 15) || ((uintptr_t)offsets & 7))
      return set_err(ctx, PN_EINVAL, "pn_udp_gather_indexed: base must be 16-byte, offsets 8-byte aligned");
    if (eth_mod16 > 15 || (eth_mod16 & 1) || avail < 96 || avail > 65536)
      return set_err(ctx, PN_EINVAL, "pn_udp_gather_indexed: eth_mod16 must be even < 16, avail in [96, 65536]");
    a.frames = (const uint8_t*)base;
    a.offs = offsets;
    a.stride = 0;
    a.frame_off = eth_mod16;
    a.avail = avail;
  }
  ug_fill(a, results, payloads, payload_cap, pay_offs, pay_lens, sub_ids, src_index, total, n);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  return ug_launch(ctx, a, (hipStream_t)stream);
}

} // extern "C"
