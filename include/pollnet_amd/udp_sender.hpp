// udp_sender.hpp — pollnet's UDP send surface (EfviUdpSender, Efvi.h:339-650) over GPU-built batches.
//
// The reference makes one sender object per destination: init builds the 42 header bytes once (init_udp_pkt,
// Efvi.h:597-609) into every pkt_buf of a 128 x 2-KiB TX ring (:436-440), and write() patches the lengths and the
// IPv4 checksum, copies the payload behind them and hands the frame to the NIC from the next buffer
// (:470-478).  GpuUdpSender holds up to PN_UDP_MAX_CHANNELS such destinations ("channels") and one ring in the
// same pkt_buf layout: write() queues a message, flush() builds the whole queued batch on the GPU
// (pn_udp_build) straight into the ring's next buffers -- wrapping at n_buf as Efvi.h:478 does -- and calls
//   sink(const uint8_t* eth, uint32_t frame_len, uint32_t buf_index)
// once per built frame, in write order: where ef_vi_transmit_ctpio / _fallback go.  buildDevice() is the same for
// messages that already lie in GPU memory.  There is no ARP or route lookup (Efvi.h:353-370): a unicast channel
// is given its destination MAC.
// Errors follow the reference: const char* (nullptr = ok).
#pragma once

#include <arpa/inet.h>
#include <netinet/in.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../pollnet_amd.h"

namespace pollnet_amd {

// EfviUdpSender::init's header (Efvi.h:344-378, 403-404) for one destination: init_udp_pkt (:597-609) with
// ci_ip4_hdr_init (:623-636: IHL 5, tos 0, tot_len 0, id 0, frag_off 0x0040 as stored = DF, ttl 64, protocol 17,
// check 0) and ci_udp_hdr_init (:638-644: ports, len htons(8), check 0).  A destination whose first octet is >= 224
// gets the multicast MAC 01:00:5e + the address's low 23 bits (:371-378) whatever dest_mac says; a unicast one
// needs dest_mac.  False: a bad address, or a unicast destination without a MAC.
inline bool udp_sender_template(pn_udp_channel* out, const char* local_ip, uint16_t local_port, const uint8_t* local_mac,
                                const char* dest_ip, uint16_t dest_port, const uint8_t* dest_mac) {
  struct in_addr la, da;
  if (!out || !local_ip || !dest_ip || !local_mac) return false;
  if (inet_pton(AF_INET, local_ip, &la) != 1 || inet_pton(AF_INET, dest_ip, &da) != 1) return false;
  uint8_t dmac[6];
  if ((0xff & da.s_addr) < 224) { // unicast
    if (!dest_mac) return false;
    std::memcpy(dmac, dest_mac, 6);
  } else { // multicast
    dmac[0] = 0x1;
    dmac[1] = 0;
    dmac[2] = 0x5e;
    dmac[3] = 0x7f & (da.s_addr >> 8);
    dmac[4] = 0xff & (da.s_addr >> 16);
    dmac[5] = 0xff & (da.s_addr >> 24);
  }
  std::memset(out, 0, sizeof(*out));
  uint8_t* h = out->hdr;
  std::memcpy(h, dmac, 6);
  std::memcpy(h + 6, local_mac, 6);
  h[12] = 0x08;
  h[13] = 0x00;
  h[14] = 0x45;
  h[20] = 0x40; // ip_frag_off_be16 = 0x0040
  h[22] = 64;
  h[23] = IPPROTO_UDP;
  std::memcpy(h + 26, &la.s_addr, 4);
  std::memcpy(h + 30, &da.s_addr, 4);
  const uint16_t sp = htons(local_port), dp = htons(dest_port), ul = htons(8);
  std::memcpy(h + 34, &sp, 2);
  std::memcpy(h + 36, &dp, 2);
  std::memcpy(h + 38, &ul, 2);
  return true;
}

} // namespace pollnet_amd

#ifndef PN_UDP_SENDER_TEMPLATE_ONLY
#include <hip/hip_runtime.h>

namespace pollnet_amd {

class GpuUdpSender {
 public:
  static constexpr uint32_t kFrameOff = 8; // sizeof(ef_addr): pkt_buf::post_addr (Efvi.h:588-594)

  GpuUdpSender() = default;
  GpuUdpSender(const GpuUdpSender&) = delete;
  GpuUdpSender& operator=(const GpuUdpSender&) = delete;
  ~GpuUdpSender() { destruct(); }

  // device: GPU ordinal; max_batch: messages one flush / buildDevice takes (<= n_buf, so that no frame is
  // overwritten before its sink call); n_buf x pkt_buf_size: the TX ring, Efvi's N_BUF and PKT_BUF_SIZE
  // (Efvi.h:646-647) by default.  The ring and the staging of payloads and index arrays are pinned host memory the
  // kernel reads and writes in place.
  const char* init(int device, uint32_t max_batch, uint32_t n_buf = 128, uint32_t pkt_buf_size = 2048) {
    destruct();
    if (max_batch == 0 || n_buf == 0 || max_batch > n_buf) return "max_batch must be in [1, n_buf]";
    if ((pkt_buf_size & 15) || pkt_buf_size < kFrameOff + 96 || pkt_buf_size > 65536)
      return "pkt_buf_size must be a multiple of 16 in [104, 65536]";
    if (pn_open(device, &ctx_)) return pn_last_error(nullptr);
    cap_ = max_batch;
    n_buf_ = n_buf;
    size_ = pkt_buf_size;
    max_pay_ = pkt_buf_size - kFrameOff - 42;
    if (max_pay_ > 65535 - 42) max_pay_ = 65535 - 42;
    if (hipSetDevice(device) != hipSuccess) return "hipSetDevice failed";
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return "hipStreamCreate failed";
    stage_bytes_ = ((size_t)max_batch * max_pay_ + 15) & ~(size_t)15;
    if (hipHostMalloc((void**)&ring_, (size_t)n_buf * pkt_buf_size, hipHostMallocDefault) != hipSuccess)
      return "hipHostMalloc(ring) failed";
    std::memset(ring_, 0, (size_t)n_buf * pkt_buf_size);
    if (hipHostMalloc((void**)&stage_, stage_bytes_, hipHostMallocDefault) != hipSuccess)
      return "hipHostMalloc(payload staging) failed";
    if (hipHostMalloc((void**)&offs_, sizeof(uint64_t) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&chans_, sizeof(uint32_t) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&lens_, sizeof(uint16_t) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&flens_, sizeof(uint16_t) * (size_t)max_batch, hipHostMallocDefault) != hipSuccess)
      return "hipHostMalloc(index arrays) failed";
    return nullptr;
  }

  // One more destination, its header built as EfviUdpSender::init builds it (udp_sender_template).  Returns the
  // channel's index, or -1: a bad address, a unicast destination without a MAC, or PN_UDP_MAX_CHANNELS in use.
  // Takes effect at the next flush / buildDevice.
  int addChannel(const char* local_ip, uint16_t local_port, const uint8_t* local_mac, const char* dest_ip,
                 uint16_t dest_port, const uint8_t* dest_mac /* may be null for multicast */) {
    if (chan_tbl_.size() >= PN_UDP_MAX_CHANNELS) return -1;
    pn_udp_channel c;
    if (!udp_sender_template(&c, local_ip, local_port, local_mac, dest_ip, dest_port, dest_mac)) return -1;
    chan_tbl_.push_back(c);
    dirty_ = true;
    return (int)chan_tbl_.size() - 1;
  }
  uint32_t channelCount() const { return (uint32_t)chan_tbl_.size(); }
  const pn_udp_channel& channel(int i) const { return chan_tbl_[(size_t)i]; }

  // PN_UB_EFVI (default: byte for byte what EfviUdpSender::write leaves), PN_UB_PLAIN or PN_UB_CSUM
  const char* setMode(uint32_t mode) {
    if (mode != PN_UB_EFVI && mode != PN_UB_PLAIN && mode != PN_UB_CSUM) return "unknown mode";
    mode_ = mode;
    return nullptr;
  }

  // EfviUdpSender::write (Efvi.h:470-478), queued: the message is copied into the staging buffer.  False: the
  // batch is full (flush first), no such channel, or the message does not fit a pkt_buf.
  bool write(int chan, const void* data, uint32_t size) {
    if (count_ >= cap_ || chan < 0 || (size_t)chan >= chan_tbl_.size() || size > max_pay_ || (size && !data)) return false;
    offs_[count_] = staged_;
    lens_[count_] = (uint16_t)size;
    chans_[count_] = (uint32_t)chan;
    if (size) std::memcpy(stage_ + staged_, data, size);
    staged_ += size;
    count_++;
    return true;
  }
  uint32_t queued() const { return count_; }

  // Builds the queued batch into the ring from bufIndex() on and calls sink once per frame, in write order.
  template <class Sink>
  const char* flush(Sink&& sink) {
    const uint32_t n = count_;
    const uint64_t bytes = staged_;
    count_ = 0;
    staged_ = 0;
    return run(stage_, bytes, offs_, lens_, chans_, n, sink);
  }

  // The same for n <= max_batch messages already in GPU memory: payloads_dev (16-byte aligned) holds
  // payload_bytes bytes; offs / lens / chans are pinned host (or device) memory as pn_udp_build takes them
  // (chans may be null: channel 0).  A message pn_udp_build refuses takes its buffer but gets no sink call.
  template <class Sink>
  const char* buildDevice(const void* payloads_dev, uint64_t payload_bytes, const uint64_t* offs, const uint16_t* lens,
                          const uint32_t* chans, uint32_t n, Sink&& sink) {
    if (n > cap_) return "buildDevice: n exceeds max_batch";
    return run(payloads_dev, payload_bytes, offs, lens, chans, n, sink);
  }

  uint32_t bufIndex() const { return buf_index_; } // the buffer the next frame goes into (s.x2.buf_index)
  uint8_t* ring() { return ring_; }                // n_buf pkt_bufs; the host owns each one's first 8 bytes (post_addr)
  uint32_t nBuf() const { return n_buf_; }
  uint32_t pktBufSize() const { return size_; }
  uint32_t maxPayload() const { return max_pay_; }
  pn_ctx* ctx() { return ctx_; }

 private:
  template <class Sink>
  const char* run(const void* pay, uint64_t pay_bytes, const uint64_t* offs, const uint16_t* lens, const uint32_t* chans,
                  uint32_t n, Sink& sink) {
    if (n == 0) return nullptr;
    if (!ctx_) return "not initialised";
    if (chan_tbl_.empty()) return "no channels";
    if (dirty_) { // nothing of this sender is in flight between calls
      if (pn_udp_set_channels(ctx_, chan_tbl_.data(), (uint32_t)chan_tbl_.size())) return pn_last_error(ctx_);
      dirty_ = false;
    }
    // from buf_index on, wrapping at n_buf (Efvi.h:478): a wrap is two builds
    const uint32_t first = n < n_buf_ - buf_index_ ? n : n_buf_ - buf_index_;
    if (pn_udp_build(ctx_, pay, pay_bytes, offs, lens, chans, ring_ + (size_t)buf_index_ * size_, size_, kFrameOff, first,
                     mode_, flens_, stream_))
      return pn_last_error(ctx_);
    if (n > first &&
        pn_udp_build(ctx_, pay, pay_bytes, offs + first, lens + first, chans ? chans + first : nullptr, ring_, size_,
                     kFrameOff, n - first, mode_, flens_ + first, stream_)) {
      (void)hipStreamSynchronize(stream_);
      return pn_last_error(ctx_);
    }
    if (hipStreamSynchronize(stream_) != hipSuccess) return "hipStreamSynchronize failed";
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t b = (buf_index_ + i) % n_buf_;
      if (flens_[i]) sink((const uint8_t*)(ring_ + (size_t)b * size_ + kFrameOff), (uint32_t)flens_[i], b);
    }
    buf_index_ = (buf_index_ + n) % n_buf_;
    return nullptr;
  }

  void destruct() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (ring_) (void)hipHostFree(ring_);
    if (stage_) (void)hipHostFree(stage_);
    if (offs_) (void)hipHostFree(offs_);
    if (chans_) (void)hipHostFree(chans_);
    if (lens_) (void)hipHostFree(lens_);
    if (flens_) (void)hipHostFree(flens_);
    if (stream_) (void)hipStreamDestroy(stream_);
    pn_close(ctx_);
    ring_ = stage_ = nullptr;
    offs_ = nullptr;
    chans_ = nullptr;
    lens_ = flens_ = nullptr;
    stream_ = nullptr;
    ctx_ = nullptr;
    chan_tbl_.clear();
    dirty_ = false;
    count_ = buf_index_ = 0;
    staged_ = 0;
    mode_ = PN_UB_EFVI;
  }

  pn_ctx* ctx_ = nullptr;
  hipStream_t stream_ = nullptr;
  uint8_t* ring_ = nullptr;
  uint8_t* stage_ = nullptr;
  uint64_t* offs_ = nullptr;
  uint32_t* chans_ = nullptr;
  uint16_t* lens_ = nullptr;
  uint16_t* flens_ = nullptr;
  size_t stage_bytes_ = 0;
  uint64_t staged_ = 0;
  uint32_t cap_ = 0, n_buf_ = 0, size_ = 0, max_pay_ = 0, count_ = 0, buf_index_ = 0;
  uint32_t mode_ = PN_UB_EFVI;
  std::vector<pn_udp_channel> chan_tbl_;
  bool dirty_ = false; // channels added since the device table was last set
};

} // namespace pollnet_amd
#endif // PN_UDP_SENDER_TEMPLATE_ONLY
