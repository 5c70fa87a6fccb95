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
// pollIndexed / pollFromIndexed take frames where RX events name them instead of a run of consecutive slots:
// frame i's Ethernet header at ring + offsets[i] (pn_udp_classify_indexed) -- for pollnet's ef_vi ring,
// EfviUdpRingLayout (rx_ring.hpp) turns a run of event ids into the offsets, eth_mod16 and avail.
// gather / gatherIndexed are poll / pollIndexed for a consumer on the GPU: instead of one handler call per datagram,
// the delivered payloads of one batch packed in order into a device buffer, with the index arrays
// GpuUdpSender::buildDevice (pn_udp_build) takes (pn_udp_gather).
// gatherBySub / gatherBySubIndexed are the same grouped by subscription (pn_udp_demux): each subscription's messages
// contiguous and in arrival order, as each of the reference's receiver objects sees only its own filter's datagrams.
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
      if (mode == GpuRx::Mode::ZeroCopy &&
          hipHostMalloc((void**)&h_offs_[b], sizeof(uint64_t) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess)
        return "hipHostMalloc(offsets) failed";
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
  // ... and those with a good header checksum whose UDP length is impossible or runs past the slot (and, in an
  // indexed poll, the frames whose offset is outside the call's alignment class: PN_UF_BADOFF)
  uint64_t droppedBadLength() const { return drop_len_; }

  template <class Handler>
  const char* poll(const uint8_t* slots, uint32_t n, Handler&& h) {
    return run(slots, n, [&](uint32_t sub, const uint8_t* data, uint16_t len) { h((int)sub, data, len); });
  }

  // EfviUdpReceiver::recvfrom (Efvi.h:241-268): the source address from data - 16, the port from data - 8
  template <class Handler>
  const char* pollFrom(const uint8_t* slots, uint32_t n, Handler&& h) {
    return run(slots, n, [&](uint32_t sub, const uint8_t* data, uint16_t len) { deliver_from(h, sub, data, len); });
  }

  // The frames where RX events put them (ZeroCopy only, as GpuRx::pollIndexed): frame i's Ethernet header at
  // ring + offsets[i], every offsets[i] % 16 == eth_mod16 (even), avail = readable bytes from each Ethernet header
  // (pn_udp_classify_indexed's contract; init's slot_stride / frame_off play no part).  `ring` is pinned host
  // memory; `offsets` is any host memory, copied chunk by chunk into two pinned buffers of max_batch entries.
  // Handler calls as poll's, in offsets order, data = ring + offsets[i] + 42.  An offset outside the class is not
  // read and counts under droppedBadLength.
  template <class Handler>
  const char* pollIndexed(const uint8_t* ring, const uint64_t* offsets, uint32_t n, uint32_t eth_mod16, uint32_t avail,
                          Handler&& h) {
    return run_indexed(ring, offsets, n, eth_mod16, avail,
                       [&](uint32_t sub, const uint8_t* data, uint16_t len) { h((int)sub, data, len); });
  }
  template <class Handler>
  const char* pollFromIndexed(const uint8_t* ring, const uint64_t* offsets, uint32_t n, uint32_t eth_mod16,
                              uint32_t avail, Handler&& h) {
    return run_indexed(ring, offsets, n, eth_mod16, avail,
                       [&](uint32_t sub, const uint8_t* data, uint16_t len) { deliver_from(h, sub, data, len); });
  }

  // What a gather leaves on the device: message j (the j-th delivered frame of the batch, in ring / offsets order)
  // is lens[j] bytes at payloads + offs[j], 16-byte aligned and zero-padded to a multiple of 16, for subscription
  // subs[j], from frame src_index[j].  n_bytes is the room the n_msgs messages need; the first n_fit were copied
  // (all of them: the receiver's buffer holds max_batch datagrams of the largest size the layout allows).  The
  // pointers are device pointers into the receiver's own buffers, valid until its next gather or init.
  struct Gathered {
    const uint8_t* payloads;
    const uint64_t* offs;
    const uint16_t* lens;
    const uint32_t* subs;
    const uint32_t* src_index;
    uint32_t n_msgs, n_fit;
    uint64_t n_bytes;
  };

  // One batch of n <= max_batch slots: pn_udp_classify + pn_udp_gather on the receiver's stream, into device buffers
  // allocated at the first call; waits for the stream and reads the total back through pinned memory.  `slots` is
  // read by the GPU where it lies, in either mode: pinned host memory or device memory.  The handler surface's drop
  // counters are not touched: no record reaches the host.
  const char* gather(const uint8_t* slots, uint32_t n, Gathered* out) {
    if (const char* e = gather_begin(n, stride_ - off_, out)) return e;
    if (n == 0 || subs_.empty()) return nullptr;
    if (pn_udp_classify(ctx_, slots, stride_, off_, n, g_.res, stream_)) return pn_last_error(ctx_);
    if (pn_udp_gather(ctx_, slots, stride_, off_, n, g_.res, g_.pay, g_.pay_cap, g_.offs, g_.lens, g_.subs, g_.src,
                      g_.total, stream_))
      return pn_last_error(ctx_);
    return gather_end(out);
  }

  // The same for frames named by offsets (pn_udp_classify_indexed's contract; `offsets` is any host memory, copied
  // into a pinned buffer; `ring` pinned host or device memory).  The payload buffer holds max_batch datagrams of
  // avail - 42 bytes.
  const char* gatherIndexed(const uint8_t* ring, const uint64_t* offsets, uint32_t n, uint32_t eth_mod16, uint32_t avail,
                            Gathered* out) {
    if (avail < 96 || avail > 65536) return "gatherIndexed: avail must be in [96, 65536]";
    if (const char* e = gather_begin(n, avail, out)) return e;
    if (n == 0 || subs_.empty()) return nullptr;
    if (!offsets) return "gatherIndexed: offsets is NULL";
    std::memcpy(g_.h_offs, offsets, sizeof(uint64_t) * n); // the previous gather has finished: it was waited for
    if (pn_udp_classify_indexed(ctx_, ring, g_.h_offs, eth_mod16, n, avail, g_.res, stream_)) return pn_last_error(ctx_);
    if (pn_udp_gather_indexed(ctx_, ring, g_.h_offs, eth_mod16, n, avail, g_.res, g_.pay, g_.pay_cap, g_.offs, g_.lens,
                              g_.subs, g_.src, g_.total, stream_))
      return pn_last_error(ctx_);
    return gather_end(out);
  }

  // What a gatherBySub leaves on the device: Gathered's fields with the messages stably sorted by subscription, and
  // sub_first / sub_bytes (subCount() + 1 entries each): subscription s owns messages [sub_first[s], sub_first[s+1])
  // and bytes [sub_bytes[s], sub_bytes[s+1]) of payloads.  With n == 0 or no subscription every field is zero.
  struct GatheredBySub : Gathered {
    const uint32_t* sub_first;
    const uint64_t* sub_bytes;
  };

  // gather with the output grouped by subscription: pn_udp_classify + pn_udp_demux on the receiver's stream, n_subs =
  // the receiver's own subscription count.  The drop counters are not touched.
  const char* gatherBySub(const uint8_t* slots, uint32_t n, GatheredBySub* out) {
    if (!out) return "gatherBySub: out is NULL";
    *out = GatheredBySub{};
    if (const char* e = gather_begin(n, stride_ - off_, out)) return e;
    if (n == 0 || subs_.empty()) return nullptr;
    if (pn_udp_classify(ctx_, slots, stride_, off_, n, g_.res, stream_)) return pn_last_error(ctx_);
    if (pn_udp_demux(ctx_, slots, stride_, off_, n, g_.res, (uint32_t)subs_.size(), g_.pay, g_.pay_cap, g_.offs, g_.lens,
                     g_.subs, g_.src, g_.sub_first, g_.sub_bytes, g_.total, stream_))
      return pn_last_error(ctx_);
    return by_sub_end(out);
  }

  // gatherIndexed with the output grouped by subscription (pn_udp_classify_indexed + pn_udp_demux_indexed).
  const char* gatherBySubIndexed(const uint8_t* ring, const uint64_t* offsets, uint32_t n, uint32_t eth_mod16,
                                 uint32_t avail, GatheredBySub* out) {
    if (!out) return "gatherBySubIndexed: out is NULL";
    *out = GatheredBySub{};
    if (avail < 96 || avail > 65536) return "gatherBySubIndexed: avail must be in [96, 65536]";
    if (const char* e = gather_begin(n, avail, out)) return e;
    if (n == 0 || subs_.empty()) return nullptr;
    if (!offsets) return "gatherBySubIndexed: offsets is NULL";
    std::memcpy(g_.h_offs, offsets, sizeof(uint64_t) * n); // the previous gather has finished: it was waited for
    if (pn_udp_classify_indexed(ctx_, ring, g_.h_offs, eth_mod16, n, avail, g_.res, stream_)) return pn_last_error(ctx_);
    if (pn_udp_demux_indexed(ctx_, ring, g_.h_offs, eth_mod16, n, avail, g_.res, (uint32_t)subs_.size(), g_.pay,
                             g_.pay_cap, g_.offs, g_.lens, g_.subs, g_.src, g_.sub_first, g_.sub_bytes, g_.total, stream_))
      return pn_last_error(ctx_);
    return by_sub_end(out);
  }

  pn_ctx* ctx() { return ctx_; }

 private:
  // The gather's buffers: device memory but the total and the offsets (pinned).  Owned by this member, so that it
  // frees them with the receiver; sized for (max_batch, avail) and allocated again when a call needs more.
  struct GatherBufs {
    pn_udp_result* res = nullptr;
    uint8_t* pay = nullptr;
    uint64_t pay_cap = 0;
    uint64_t* offs = nullptr;
    uint16_t* lens = nullptr;
    uint32_t* subs = nullptr;
    uint32_t* src = nullptr;
    uint32_t* sub_first = nullptr; // gatherBySub: PN_UDP_MAX_SUBS + 1 entries each
    uint64_t* sub_bytes = nullptr;
    uint64_t* h_offs = nullptr;
    pn_udp_gather_total* total = nullptr;
    uint32_t batch = 0;
    GatherBufs() = default;
    GatherBufs(const GatherBufs&) = delete;
    GatherBufs& operator=(const GatherBufs&) = delete;
    ~GatherBufs() { release(); }
    void release() {
      if (res) (void)hipFree(res);
      if (pay) (void)hipFree(pay);
      if (offs) (void)hipFree(offs);
      if (lens) (void)hipFree(lens);
      if (subs) (void)hipFree(subs);
      if (src) (void)hipFree(src);
      if (sub_first) (void)hipFree(sub_first);
      if (sub_bytes) (void)hipFree(sub_bytes);
      if (h_offs) (void)hipHostFree(h_offs);
      if (total) (void)hipHostFree(total);
      res = nullptr, pay = nullptr, offs = nullptr, lens = nullptr, subs = nullptr, src = nullptr, h_offs = nullptr;
      total = nullptr, sub_first = nullptr, sub_bytes = nullptr;
      pay_cap = 0, batch = 0;
    }
  };

  // Checks, the subscriptions, and buffers for `n` frames of `avail` readable bytes; *out zeroed.
  const char* gather_begin(uint32_t n, uint32_t avail, Gathered* out) {
    if (!ctx_) return "gather: init first";
    if (!out) return "gather: out is NULL";
    *out = Gathered{};
    if (n > cap_) return "gather: n must not exceed max_batch";
    if (n == 0 || subs_.empty()) return nullptr;
    if (pn_sync(ctx_)) return pn_last_error(ctx_); // nothing is in flight; makes the ctx's device current
    if (dirty_) { // nothing of this receiver is in flight between calls
      if (pn_udp_set_subs(ctx_, subs_.data(), (uint32_t)subs_.size())) return pn_last_error(ctx_);
      dirty_ = false;
    }
    const uint64_t want = (uint64_t)cap_ * ((avail - 42 + 15) & ~15u);
    if (g_.batch != cap_ || g_.pay_cap < want) {
      g_.release();
      const size_t b = cap_;
      if (hipMalloc((void**)&g_.res, sizeof(pn_udp_result) * b) != hipSuccess ||
          hipMalloc((void**)&g_.pay, want) != hipSuccess || hipMalloc((void**)&g_.offs, sizeof(uint64_t) * b) != hipSuccess ||
          hipMalloc((void**)&g_.lens, sizeof(uint16_t) * b) != hipSuccess ||
          hipMalloc((void**)&g_.subs, sizeof(uint32_t) * b) != hipSuccess ||
          hipMalloc((void**)&g_.src, sizeof(uint32_t) * b) != hipSuccess ||
          hipMalloc((void**)&g_.sub_first, sizeof(uint32_t) * (PN_UDP_MAX_SUBS + 1)) != hipSuccess ||
          hipMalloc((void**)&g_.sub_bytes, sizeof(uint64_t) * (PN_UDP_MAX_SUBS + 1)) != hipSuccess ||
          hipHostMalloc((void**)&g_.h_offs, sizeof(uint64_t) * b, hipHostMallocDefault) != hipSuccess ||
          hipHostMalloc((void**)&g_.total, sizeof(pn_udp_gather_total), hipHostMallocDefault) != hipSuccess) {
        g_.release();
        return "gather: allocating the device buffers failed";
      }
      g_.pay_cap = want;
      g_.batch = cap_;
    }
    return nullptr;
  }

  const char* gather_end(Gathered* out) {
    if (hipStreamSynchronize(stream_) != hipSuccess) return "hipStreamSynchronize failed";
    out->payloads = g_.pay;
    out->offs = g_.offs;
    out->lens = g_.lens;
    out->subs = g_.subs;
    out->src_index = g_.src;
    out->n_msgs = g_.total->n_msgs;
    out->n_fit = g_.total->n_fit;
    out->n_bytes = g_.total->n_bytes;
    return nullptr;
  }

  const char* by_sub_end(GatheredBySub* out) {
    if (const char* e = gather_end(out)) return e;
    out->sub_first = g_.sub_first;
    out->sub_bytes = g_.sub_bytes;
    return nullptr;
  }

  // EfviUdpReceiver::recvfrom (Efvi.h:251-255): the source address from data - 16, the port from data - 8
  template <class Handler>
  static void deliver_from(Handler& h, uint32_t sub, const uint8_t* data, uint16_t len) {
    struct sockaddr_in src_addr;
    std::memset(&src_addr, 0, sizeof(src_addr));
    src_addr.sin_family = AF_INET;
    std::memcpy(&src_addr.sin_addr.s_addr, data - 16, 4);
    std::memcpy(&src_addr.sin_port, data - 8, 2);
    h((int)sub, data, len, (const struct sockaddr_in&)src_addr);
  }

  // What every poll checks before its first launch.
  const char* prepare(const uint8_t* ring) {
    if (mode_ == GpuRx::Mode::ZeroCopy) {
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, ring) != hipSuccess || attr.type != hipMemoryTypeHost)
        return "zero-copy ring must be pinned host memory (hipHostMalloc / hipHostRegister)";
    }
    if (dirty_) { // nothing of this receiver is in flight between polls
      if (pn_udp_set_subs(ctx_, subs_.data(), (uint32_t)subs_.size())) return pn_last_error(ctx_);
      dirty_ = false;
    }
    return nullptr;
  }

  template <class Deliver>
  const char* run(const uint8_t* slots, uint32_t n, Deliver&& deliver) {
    if (n == 0 || subs_.empty()) return nullptr;
    if (const char* e = prepare(slots)) return e;
    const char* e = run_chunks(
        n, [&](uint32_t k) { return launch(slots, n, k); },
        [&](uint32_t i) { return slots + (size_t)i * stride_ + off_; }, deliver);
    if (e) (void)hipStreamSynchronize(stream_); // leave no chunk in flight
    return e;
  }

  template <class Deliver>
  const char* run_indexed(const uint8_t* ring, const uint64_t* offsets, uint32_t n, uint32_t eth_mod16, uint32_t avail,
                          Deliver&& deliver) {
    if (mode_ != GpuRx::Mode::ZeroCopy) return "pollIndexed needs Mode::ZeroCopy";
    if (n == 0 || subs_.empty()) return nullptr;
    if (!offsets) return "pollIndexed: offsets is NULL";
    if (const char* e = prepare(ring)) return e;
    auto launch_k = [&](uint32_t k) -> const char* {
      const uint32_t base = k * cap_, m = std::min(cap_, n - base), b = k & 1;
      std::memcpy(h_offs_[b], offsets + base, sizeof(uint64_t) * m); // buffer b is free: chunk k-2 was delivered
      if (pn_udp_classify_indexed(ctx_, ring, h_offs_[b], eth_mod16, m, avail, h_res_[b], stream_))
        return pn_last_error(ctx_);
      if (hipEventRecord(done_[b], stream_) != hipSuccess) return "hipEventRecord failed";
      return nullptr;
    };
    const char* e = run_chunks(n, launch_k, [&](uint32_t i) { return ring + offsets[i]; }, deliver);
    if (e) (void)hipStreamSynchronize(stream_);
    return e;
  }

  // The chunk pipeline of every poll: chunk k+1 is launched before chunk k is waited for and delivered.
  // eth_of(i): frame i's Ethernet header.
  template <class LaunchK, class EthOf, class Deliver>
  const char* run_chunks(uint32_t n, LaunchK&& launch_k, EthOf&& eth_of, Deliver& deliver) {
    const uint32_t chunks = (n + cap_ - 1) / cap_;
    if (const char* e = launch_k(0)) return e;
    for (uint32_t k = 0; k < chunks; k++) {
      if (k + 1 < chunks)
        if (const char* e = launch_k(k + 1)) return e;
      if (hipEventSynchronize(done_[k & 1]) != hipSuccess) return "hipEventSynchronize failed";
      const uint32_t base = k * cap_, m = std::min(cap_, n - base);
      const pn_udp_result* res = h_res_[k & 1];
      for (uint32_t i = 0; i < m; i++) {
        const pn_udp_result& r = res[i];
        if (r.flags & PN_UF_BADOFF) { // indexed polls only: an offset outside the class, nothing of it was read
          drop_len_++;
          continue;
        }
        if (!(r.flags & PN_UF_MATCH)) continue;
        if (PN_UDP_DELIVER(r.flags)) {
          deliver(r.sub_id, eth_of(base + i) + r.payload_off, r.payload_len);
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
      if (h_offs_[b]) (void)hipHostFree(h_offs_[b]);
      h_offs_[b] = nullptr;
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
  uint64_t* h_offs_[2] = {nullptr, nullptr}; // ZeroCopy: pinned offsets the indexed kernel reads
  hipEvent_t done_[2] = {nullptr, nullptr};
  uint32_t stride_ = 0, off_ = 0, cap_ = 0;
  std::vector<pn_udp_sub> subs_;
  bool dirty_ = false; // subscriptions added since the device table was last set
  uint64_t drop_ip_ = 0, drop_udp_ = 0, drop_len_ = 0;
  GatherBufs g_; // gather / gatherIndexed only
};

} // namespace pollnet_amd
