// udp_receiver.hpp — pollnet's UDP receive surface (EfviUdpReceiver / SocketUdpReceiver, Efvi.h:132-273,
// Socket.h:394-493) over GPU-filtered batches.
//
// The reference makes one receiver object, and one NIC filter, per (dest_ip, dest_port)
// (ef_filter_spec_set_ip4_local, Efvi.h:143-156) and reads one event per call.  GpuUdpReceiver holds up to
// PN_UDP_MAX_SUBS such subscriptions and takes a run of ring slots that carries everything on the wire:
// poll() classifies it with pn_udp_classify in chunks of max_batch (chunk k+1 on the GPU while chunk k is
// delivered) and hands every PN_UDP_DELIVER frame -- subscribed, IPv4 header checksum good, UDP checksum good or
// not sent: what a NIC reports as EF_EVENT_TYPE_RX -- to the handler in ring order, with the reference's own
// arithmetic (Efvi.h:198-200, 251-255):
//   poll:      h(int sub, const uint8_t* data, uint16_t len)            data = eth + 42, len = ntohs(udp->len) - 8
//   pollFrom:  h(int sub, const uint8_t* data, uint16_t len, const sockaddr_in& src)
// `data` points into the caller's ring (zero-copy, valid during the call).  Frames of no subscription are never
// touched by the host.  Subscribed frames dropped for a bad IPv4 or UDP checksum are counted, as the
// reference's applications count misses.
// Errors follow the reference: const char* (nullptr = ok).
#pragma once

#include <arpa/inet.h>
#include <netinet/in.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gpu_rx.hpp"

namespace pollnet_amd {

class GpuUdpReceiver {
 public:
  GpuUdpReceiver() = default;
  GpuUdpReceiver(const GpuUdpReceiver&) = delete;
  GpuUdpReceiver& operator=(const GpuUdpReceiver&) = delete;
  ~GpuUdpReceiver() { destruct(); }

  // device: GPU ordinal; slot_stride / frame_off: the ring layout (pn_udp_classify's contract); max_batch: the
  // chunk one launch classifies (two chunks are in flight at once).
  // Copy: the slots are copied H2D and the records back (any host memory); ZeroCopy: the kernel reads the slots
  // from pinned host memory and writes the records to pinned memory -- only the header line of a frame for
  // somebody else crosses the bus.
  const char* init(int device, uint32_t slot_stride, uint32_t frame_off, uint32_t max_batch,
                   GpuRx::Mode mode = GpuRx::Mode::ZeroCopy) {
    destruct();
    if (max_batch == 0) return "max_batch must be > 0";
    if (pn_open(device, &ctx_)) return pn_last_error(nullptr);
    stride_ = slot_stride;
    off_ = frame_off;
    cap_ = max_batch;
    mode_ = mode;
    if (hipSetDevice(device) != hipSuccess) return "hipSetDevice failed";
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return "hipStreamCreate failed";
    for (int b = 0; b < 2; b++) {
      if (mode == GpuRx::Mode::Copy) {
        if (hipMalloc(&d_frames_[b], (size_t)slot_stride * max_batch) != hipSuccess) return "hipMalloc(frames) failed";
        if (hipMalloc((void**)&d_res_[b], sizeof(pn_udp_result) * (size_t)max_batch) != hipSuccess)
          return "hipMalloc(results) failed";
      }
      if (hipHostMalloc((void**)&h_res_[b], sizeof(pn_udp_result) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess)
        return "hipHostMalloc(results) failed";
      if (hipEventCreateWithFlags(&done_[b], hipEventDisableTiming) != hipSuccess) return "hipEventCreate failed";
    }
    return nullptr;
  }

  // EfviUdpReceiver::init's filter (Efvi.h:143-156) for one more (dest_ip, dest_port).  Returns the
  // subscription's index (the handler's `sub`), or -1: a bad address, a pair subscribed already, or
  // PN_UDP_MAX_SUBS in use.  Takes effect at the next poll.
  int subscribe(const char* dest_ip, uint16_t dest_port) {
    if (subs_.size() >= PN_UDP_MAX_SUBS) return -1;
    pn_udp_sub s{};
    if (inet_pton(AF_INET, dest_ip, &s.dst_ip) != 1) return -1;
    s.dst_port = htons(dest_port);
    for (const pn_udp_sub& q : subs_)
      if (q.dst_ip == s.dst_ip && q.dst_port == s.dst_port) return -1;
    subs_.push_back(s);
    dirty_ = true;
    return (int)subs_.size() - 1;
  }
  uint32_t subCount() const { return (uint32_t)subs_.size(); }

  // pn_set_verify: false = no UDP checksum is computed (PN_UF_UDP_UNCHECKED frames are delivered)
  const char* setVerify(bool on) { return pn_set_verify(ctx_, on ? 1 : 0) ? pn_last_error(ctx_) : nullptr; }

  // Subscribed frames not delivered because the IPv4 header checksum / the UDP checksum failed (a frame failing
  // both counts under the IP one), since init.
  uint64_t droppedBadIpCsum() const { return drop_ip_; }
  uint64_t droppedBadUdpCsum() const { return drop_udp_; }
  // ... and those with a good header checksum whose UDP length is impossible or runs past the slot
  uint64_t droppedBadLength() const { return drop_len_; }

  template <class Handler>
  const char* poll(const uint8_t* slots, uint32_t n, Handler&& h) {
    return run(slots, n, [&](uint32_t sub, const uint8_t* data, uint16_t len) { h((int)sub, data, len); });
  }

  // EfviUdpReceiver::recvfrom (Efvi.h:241-268): the source address from data - 16, the port from data - 8
  template <class Handler>
  const char* pollFrom(const uint8_t* slots, uint32_t n, Handler&& h) {
    return run(slots, n, [&](uint32_t sub, const uint8_t* data, uint16_t len) {
      struct sockaddr_in src_addr;
      std::memset(&src_addr, 0, sizeof(src_addr));
      src_addr.sin_family = AF_INET;
      std::memcpy(&src_addr.sin_addr.s_addr, data - 16, 4);
      std::memcpy(&src_addr.sin_port, data - 8, 2);
      h((int)sub, data, len, (const struct sockaddr_in&)src_addr);
    });
  }

  pn_ctx* ctx() { return ctx_; }

 private:
  template <class Deliver>
  const char* run(const uint8_t* slots, uint32_t n, Deliver&& deliver) {
    if (n == 0 || subs_.empty()) return nullptr;
    if (mode_ == GpuRx::Mode::ZeroCopy) {
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, slots) != hipSuccess || attr.type != hipMemoryTypeHost)
        return "zero-copy ring must be pinned host memory (hipHostMalloc / hipHostRegister)";
    }
    if (dirty_) { // nothing of this receiver is in flight between polls
      if (pn_udp_set_subs(ctx_, subs_.data(), (uint32_t)subs_.size())) return pn_last_error(ctx_);
      dirty_ = false;
    }
    const char* e = run_chunks(slots, n, deliver);
    if (e) (void)hipStreamSynchronize(stream_); // leave no chunk in flight
    return e;
  }

  template <class Deliver>
  const char* run_chunks(const uint8_t* slots, uint32_t n, Deliver& deliver) {
    const uint32_t chunks = (n + cap_ - 1) / cap_;
    if (const char* e = launch(slots, n, 0)) return e;
    for (uint32_t k = 0; k < chunks; k++) {
      if (k + 1 < chunks)
        if (const char* e = launch(slots, n, k + 1)) return e;
      if (hipEventSynchronize(done_[k & 1]) != hipSuccess) return "hipEventSynchronize failed";
      const uint32_t base = k * cap_, m = std::min(cap_, n - base);
      const pn_udp_result* res = h_res_[k & 1];
      for (uint32_t i = 0; i < m; i++) {
        const pn_udp_result& r = res[i];
        if (!(r.flags & PN_UF_MATCH)) continue;
        if (PN_UDP_DELIVER(r.flags)) {
          const uint8_t* data = slots + (size_t)(base + i) * stride_ + off_ + r.payload_off;
          deliver(r.sub_id, data, r.payload_len);
        } else if (!(r.flags & PN_UF_IP_OK)) {
          drop_ip_++;
        } else if (!(r.flags & (PN_UF_LEN_BAD | PN_UF_TRUNC))) {
          drop_udp_++; // checkable, a checksum sent, and it did not verify
        } else {
          drop_len_++;
        }
      }
    }
    return nullptr;
  }

  const char* launch(const uint8_t* slots, uint32_t n, uint32_t k) {
    const uint32_t base = k * cap_, m = std::min(cap_, n - base), b = k & 1;
    const uint8_t* src = slots + (size_t)base * stride_;
    if (mode_ == GpuRx::Mode::ZeroCopy) {
      if (pn_udp_classify(ctx_, src, stride_, off_, m, h_res_[b], stream_)) return pn_last_error(ctx_);
    } else {
      if (hipMemcpyAsync(d_frames_[b], src, (size_t)stride_ * m, hipMemcpyHostToDevice, stream_) != hipSuccess)
        return "hipMemcpyAsync H2D failed";
      if (pn_udp_classify(ctx_, d_frames_[b], stride_, off_, m, d_res_[b], stream_)) return pn_last_error(ctx_);
      if (hipMemcpyAsync(h_res_[b], d_res_[b], sizeof(pn_udp_result) * m, hipMemcpyDeviceToHost, stream_) != hipSuccess)
        return "hipMemcpyAsync D2H failed";
    }
    if (hipEventRecord(done_[b], stream_) != hipSuccess) return "hipEventRecord failed";
    return nullptr;
  }

  void destruct() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (int b = 0; b < 2; b++) {
      if (done_[b]) (void)hipEventDestroy(done_[b]);
      if (h_res_[b]) (void)hipHostFree(h_res_[b]);
      if (d_res_[b]) (void)hipFree(d_res_[b]);
      if (d_frames_[b]) (void)hipFree(d_frames_[b]);
      done_[b] = nullptr;
      h_res_[b] = d_res_[b] = nullptr;
      d_frames_[b] = nullptr;
    }
    if (stream_) (void)hipStreamDestroy(stream_);
    pn_close(ctx_);
    stream_ = nullptr;
    ctx_ = nullptr;
    subs_.clear();
    dirty_ = false;
    drop_ip_ = drop_udp_ = drop_len_ = 0;
  }

  pn_ctx* ctx_ = nullptr;
  hipStream_t stream_ = nullptr;
  GpuRx::Mode mode_ = GpuRx::Mode::ZeroCopy;
  void* d_frames_[2] = {nullptr, nullptr};
  pn_udp_result* d_res_[2] = {nullptr, nullptr};
  pn_udp_result* h_res_[2] = {nullptr, nullptr};
  hipEvent_t done_[2] = {nullptr, nullptr};
  uint32_t stride_ = 0, off_ = 0, cap_ = 0;
  std::vector<pn_udp_sub> subs_;
  bool dirty_ = false; // subscriptions added since the device table was last set
  uint64_t drop_ip_ = 0, drop_udp_ = 0, drop_len_ = 0;
};

} // namespace pollnet_amd
