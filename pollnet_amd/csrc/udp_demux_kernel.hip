// pn_udp_demux / pn_udp_demux_indexed: the UDP demux path -- the delivered payloads of a classified ring grouped by
// subscription, each subscription's messages contiguous and in arrival order, with pn_udp_gather's index arrays and
// the per-subscription extents.  The kernels are in udp_demux.hpp.
#include "udp_demux.hpp"

namespace {
using pn_internal::hip_err;
using pn_internal::set_err;

// The checks both entry points share: the outputs and the records.  total and the per-subscription arrays first:
// n == 0 needs nothing else.
int ud_check_outputs(pn_ctx* ctx, const char* who, uint32_t n, const void* results, uint32_t n_subs, void* payloads,
                     uint64_t payload_cap, uint64_t* pay_offs, uint16_t* pay_lens, uint32_t* sub_ids,
                     uint32_t* src_index, uint32_t* sub_first, uint64_t* sub_bytes, pn_udp_gather_total* total) {
  const std::string w(who);
  if (!total || !sub_first || !sub_bytes) return set_err(ctx, PN_EINVAL, w + ": NULL total, sub_first or sub_bytes");
  if (((uintptr_t)total & 7) || ((uintptr_t)sub_first & 3) || ((uintptr_t)sub_bytes & 7))
    return set_err(ctx, PN_EINVAL, w + ": total and sub_bytes must be 8-byte, sub_first 4-byte aligned");
  if (n_subs == 0 || n_subs > PN_UDP_MAX_SUBS) return set_err(ctx, PN_EINVAL, w + ": n_subs must be in [1, PN_UDP_MAX_SUBS]");
  if (n > PN_UDP_DEMUX_MAX_N) return set_err(ctx, PN_EINVAL, w + ": n above PN_UDP_DEMUX_MAX_N");
  if (n == 0) return PN_OK;
  if (!results || !payloads || !pay_offs || !pay_lens || !sub_ids) return set_err(ctx, PN_EINVAL, w + ": NULL buffer");
  if (((uintptr_t)results & 15) || ((uintptr_t)payloads & 15) || (payload_cap & 15) || ((uintptr_t)pay_offs & 7) ||
      ((uintptr_t)pay_lens & 1) || ((uintptr_t)sub_ids & 3) || ((uintptr_t)src_index & 3))
    return set_err(ctx, PN_EINVAL,
                   w + ": results/payloads must be 16-byte aligned, payload_cap a multiple of 16, the index arrays "
                       "aligned to their element");
  return PN_OK;
}

void ud_fill(UdArgs& a, const void* results, uint32_t n_subs, void* payloads, uint64_t payload_cap, uint64_t* pay_offs,
             uint16_t* pay_lens, uint32_t* sub_ids, uint32_t* src_index, uint32_t* sub_first, uint64_t* sub_bytes,
             pn_udp_gather_total* total, uint32_t n) {
  a.results = (const u32x4*)results;
  a.n_subs = n_subs;
  a.pay = (uint8_t*)payloads;
  a.cap = payload_cap;
  a.pay_offs = pay_offs;
  a.pay_lens = pay_lens;
  a.sub_ids = sub_ids;
  a.src_index = src_index;
  a.sub_first = sub_first;
  a.sub_bytes = sub_bytes;
  a.total = total;
  a.n = n;
}
} // namespace

extern "C" {

int pn_udp_demux(pn_ctx* ctx, const void* frames, uint32_t slot_stride, uint32_t frame_off, uint32_t n,
                 const void* results, uint32_t n_subs, void* payloads, uint64_t payload_cap, uint64_t* pay_offs,
                 uint16_t* pay_lens, uint32_t* sub_ids, uint32_t* src_index, uint32_t* sub_first, uint64_t* sub_bytes,
                 pn_udp_gather_total* total, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_demux: ctx is NULL");
  if (int rc = ud_check_outputs(ctx, "pn_udp_demux", n, results, n_subs, payloads, payload_cap, pay_offs, pay_lens,
                                sub_ids, src_index, sub_first, sub_bytes, total))
    return rc;
  UdArgs a = {};
  if (n) {
    if (!frames) return set_err(ctx, PN_EINVAL, "pn_udp_demux: NULL buffer");
    if ((uintptr_t)frames & 15) return set_err(ctx, PN_EINVAL, "pn_udp_demux: frames must be 16-byte aligned");
    if ((slot_stride & 15) || slot_stride > 65536 || (frame_off & 1) || slot_stride < frame_off + 96)
      return set_err(ctx, PN_EINVAL, "pn_udp_demux: slot_stride/frame_off violate the layout contract");
    a.frames = (const uint8_t*)frames;
    a.offs = nullptr;
    a.stride = slot_stride;
    a.frame_off = frame_off;
    a.avail = slot_stride - frame_off;
  }
  ud_fill(a, results, n_subs, payloads, payload_cap, pay_offs, pay_lens, sub_ids, src_index, sub_first, sub_bytes, total,
          n);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  return ud_launch(ctx, a, (hipStream_t)stream);
}

int pn_udp_demux_indexed(pn_ctx* ctx, const void* base, const uint64_t* offsets, uint32_t eth_mod16, uint32_t n,
                         uint32_t avail, const void* results, uint32_t n_subs, void* payloads, uint64_t payload_cap,
                         uint64_t* pay_offs, uint16_t* pay_lens, uint32_t* sub_ids, uint32_t* src_index,
                         uint32_t* sub_first, uint64_t* sub_bytes, pn_udp_gather_total* total, void* stream) {
  if (!ctx) return set_err(nullptr, PN_EINVAL, "pn_udp_demux_indexed: ctx is NULL");
  if (int rc = ud_check_outputs(ctx, "pn_udp_demux_indexed", n, results, n_subs, payloads, payload_cap, pay_offs,
                                pay_lens, sub_ids, src_index, sub_first, sub_bytes, total))
    return rc;
  UdArgs a = {};
  if (n) {
    if (!base || !offsets) return set_err(ctx, PN_EINVAL, "pn_udp_demux_indexed: NULL buffer");
    if (((uintptr_t)base & 15) || ((uintptr_t)offsets & 7))
      return set_err(ctx, PN_EINVAL, "pn_udp_demux_indexed: base must be 16-byte, offsets 8-byte aligned");
    if (eth_mod16 > 15 || (eth_mod16 & 1) || avail < 96 || avail > 65536)
      return set_err(ctx, PN_EINVAL, "pn_udp_demux_indexed: eth_mod16 must be even < 16, avail in [96, 65536]");
    a.frames = (const uint8_t*)base;
    a.offs = offsets;
    a.stride = 0;
    a.frame_off = eth_mod16;
    a.avail = avail;
  }
  ud_fill(a, results, n_subs, payloads, payload_cap, pay_offs, pay_lens, sub_ids, src_index, sub_first, sub_bytes, total,
          n);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_err(ctx, e, "hipSetDevice");
  return ud_launch(ctx, a, (hipStream_t)stream);
}

} // extern "C"
