// GpuUdpSender (include/pollnet_amd/udp_sender.hpp) against a sequential twin that restates, per channel,
// EfviUdpSender::init (the header of init_udp_pkt, Efvi.h:597-609, 623-644, the multicast MAC of :371-378, the
// cached IPv4 sum of :405-411) and EfviUdpSender::write (update_udp_pkt, :611-621, the memcpy behind the header,
// :474, frame_len, :475, and the buf_index wrap, :478) over one ring in the pkt_buf layout (:588-594, 646-647):
// the same ring bytes and the same sink calls in the same order with the same buf_index, over three flushes that
// cross the ring's wrap, a refused oversize write, and buildDevice.  Then the ring, rebuilt in PN_UB_PLAIN mode,
// goes through a GpuUdpReceiver subscribed to the same destinations: every payload arrives intact on its
// subscription.
#include <arpa/inet.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/pollnet_amd/udp_receiver.hpp"
#include "../../include/pollnet_amd/udp_sender.hpp"

using pollnet_amd::GpuUdpReceiver;
using pollnet_amd::GpuUdpSender;

static int g_fail = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      if (g_fail < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                 \
    }                                                           \
  } while (0)

namespace {

constexpr uint32_t kNBuf = 128, kBufSize = 2048; // N_BUF, PKT_BUF_SIZE (Efvi.h:646-647)

struct Dest {
  const char* local_ip;
  uint16_t local_port;
  const char* dest_ip;
  uint16_t dest_port;
  bool unicast;
};
const Dest kDests[] = {
    {"10.20.30.40", 40000, "239.1.2.3", 20001, false}, {"10.20.30.40", 40000, "239.1.2.4", 20001, false},
    {"10.20.30.40", 40001, "239.200.130.9", 20002, false}, {"192.168.7.1", 1000, "192.168.7.77", 31001, true},
    {"192.168.7.1", 1001, "10.0.0.9", 31002, true},
};
const uint8_t kLocalMac[6] = {0x00, 0x0f, 0x53, 0x10, 0x20, 0x30};
const uint8_t kPeerMac[6] = {0x3c, 0xfd, 0xfe, 0xaa, 0xbb, 0xcc};

struct SinkCall {
  size_t eth_off; // eth - ring
  uint32_t frame_len, buf_index;
  bool operator==(const SinkCall& o) const { return eth_off == o.eth_off && frame_len == o.frame_len && buf_index == o.buf_index; }
};

// One EfviUdpSender, restated: its 42 header bytes and ipsum_cache.
struct TwinChannel {
  uint8_t eth[42];
  uint32_t ipsum_cache;

  void init(const Dest& d) {
    struct in_addr la, da;
    inet_pton(AF_INET, d.local_ip, &la);
    inet_pton(AF_INET, d.dest_ip, &da);
    std::memset(eth, 0, 42);
    if ((0xff & da.s_addr) < 224) { // unicast: the ARP entry (Efvi.h:353-370)
      std::memcpy(eth, kPeerMac, 6);
    } else { // Efvi.h:371-378
      eth[0] = 1, eth[1] = 0, eth[2] = 0x5e;
      eth[3] = 0x7f & (da.s_addr >> 8);
      eth[4] = 0xff & (da.s_addr >> 16);
      eth[5] = 0xff & (da.s_addr >> 24);
    }
    std::memcpy(eth + 6, kLocalMac, 6);       // Efvi.h:604
    eth[12] = 0x08, eth[13] = 0x00;           // :603
    uint8_t* ip = eth + 14;                   // ci_ip4_hdr_init, :623-636
    ip[0] = (4u << 4) | (20 >> 2);
    ip[6] = 0x40, ip[7] = 0x00;               // frag_off 0x0040 as stored
    ip[8] = 64, ip[9] = 17;
    std::memcpy(ip + 12, &la.s_addr, 4);
    std::memcpy(ip + 16, &da.s_addr, 4);
    uint8_t* udp = ip + 20;                   // ci_udp_hdr_init, :638-644
    const uint16_t sp = htons(d.local_port), dp = htons(d.dest_port), ul = htons(8);
    std::memcpy(udp, &sp, 2);
    std::memcpy(udp + 2, &dp, 2);
    std::memcpy(udp + 4, &ul, 2);
    uint16_t w[10];                           // :405-411
    std::memcpy(w, ip, 20);
    ipsum_cache = 0;
    for (int i = 0; i < 10; i++) ipsum_cache += w[i];
    ipsum_cache = (ipsum_cache >> 16u) + (ipsum_cache & 0xffff);
    ipsum_cache += (ipsum_cache >> 16u);
  }

  // update_udp_pkt (:611-621) on a frame; plain = the IPv4 checksum by the standard fold instead (PN_UB_PLAIN)
  void update(uint8_t* frame, uint32_t paylen, bool plain) const {
    const uint16_t iplen = htons(28 + paylen), ulen = htons(8 + paylen);
    std::memcpy(frame + 16, &iplen, 2);
    uint16_t check;
    if (!plain) {
      uint32_t ipsum = ipsum_cache + iplen;
      ipsum += (ipsum >> 16u);
      check = ~ipsum & 0xffff;
    } else {
      uint16_t w[10];
      std::memcpy(w, frame + 14, 20);
      w[5] = 0;
      uint32_t s = 0;
      for (int i = 0; i < 10; i++) s += w[i];
      while (s >> 16) s = (s >> 16) + (s & 0xffff);
      check = ~s & 0xffff;
    }
    std::memcpy(frame + 24, &check, 2);
    std::memcpy(frame + 38, &ulen, 2);
  }
};

struct Twin {
  std::vector<uint8_t> ring = std::vector<uint8_t>((size_t)kNBuf * kBufSize, 0);
  std::vector<TwinChannel> chans;
  uint32_t buf_index = 0;
  bool plain = false;
  std::vector<SinkCall> calls;
  // what each buffer holds now: channel, payload
  std::vector<int> slot_chan = std::vector<int>(kNBuf, -1);
  std::vector<std::vector<uint8_t>> slot_pay = std::vector<std::vector<uint8_t>>(kNBuf);

  // EfviUdpSender::write (:470-478) of channel `chan`
  void write(int chan, const void* data, uint32_t size) {
    uint8_t* pkt = ring.data() + (size_t)buf_index * kBufSize;
    uint8_t* eth = pkt + 8; // past post_addr
    std::memcpy(eth, chans[chan].eth, 42); // the header init left in this sender's pkt_bufs (:439)
    chans[chan].update(eth, size, plain);
    std::memcpy(eth + 42, data, size); // memcpy(pkt + 1, data, size)
    calls.push_back({(size_t)(eth - ring.data()), 42 + size, buf_index});
    slot_chan[buf_index] = chan;
    slot_pay[buf_index].assign((const uint8_t*)data, (const uint8_t*)data + size);
    buf_index = (buf_index + 1) % kNBuf;
  }
  void skip() { buf_index = (buf_index + 1) % kNBuf; } // buildDevice: a refused message takes its buffer
};

void compare(const char* stage, GpuUdpSender& tx, Twin& tw, const std::vector<SinkCall>& got) {
  const size_t before = g_fail;
  CHECK(got.size() == tw.calls.size());
  for (size_t i = 0; i < got.size() && i < tw.calls.size(); i++) CHECK(got[i] == tw.calls[i]);
  size_t diff = 0, first = 0;
  for (size_t i = 0; i < tw.ring.size(); i++)
    if (tx.ring()[i] != tw.ring[i] && diff++ == 0) first = i;
  if (diff) std::printf("  ring differs in %zu bytes, first at buffer %zu + %zu\n", diff, first / kBufSize, first % kBufSize);
  CHECK(diff == 0);
  CHECK(tx.bufIndex() == tw.buf_index);
  std::printf("%s: %zu sink calls, buf_index %u%s\n", stage, got.size(), tx.bufIndex(), g_fail == (int)before ? "" : "  (FAILED)");
  tw.calls.clear();
}

} // namespace

int main() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::printf("no GPU\n");
    return 2;
  }
  GpuUdpSender tx;
  if (const char* e = tx.init(0, 100)) {
    std::printf("FAIL init: %s\n", e);
    return 1;
  }
  CHECK(tx.nBuf() == kNBuf && tx.pktBufSize() == kBufSize && tx.maxPayload() == kBufSize - 50);
  Twin tw;
  const int n_ch = (int)(sizeof(kDests) / sizeof(kDests[0]));
  for (int c = 0; c < n_ch; c++) {
    const Dest& d = kDests[c];
    CHECK(tx.addChannel(d.local_ip, d.local_port, kLocalMac, d.dest_ip, d.dest_port, d.unicast ? kPeerMac : nullptr) == c);
    TwinChannel t;
    t.init(d);
    tw.chans.push_back(t);
    CHECK(std::memcmp(tx.channel(c).hdr, t.eth, 42) == 0);
  }
  CHECK(tx.addChannel("10.0.0.1", 1, kLocalMac, "10.0.0.2", 2, nullptr) == -1); // unicast without a MAC

  std::mt19937 rng(20260);
  std::vector<uint8_t> msg(4096);
  auto fill = [&](uint32_t size) {
    for (uint32_t i = 0; i < size; i++) msg[i] = (uint8_t)rng();
  };
  const uint32_t sizes[] = {0, 1, 2, 3, 64, 65, 200, 777, 1400, 1472, 1997, 1998};
  std::vector<SinkCall> got;
  auto sink = [&](const uint8_t* eth, uint32_t frame_len, uint32_t buf_index) {
    got.push_back({(size_t)(eth - tx.ring()), frame_len, buf_index});
  };
  // `count` accepted writes through both, with refused ones in between
  auto queue = [&](uint32_t count) {
    for (uint32_t k = 0; k < count; k++) {
      const uint32_t size = k % 5 == 4 ? (uint32_t)(rng() % 1999) : sizes[(k / 2) % 12];
      const int chan = (int)(rng() % n_ch);
      fill(size);
      if (k % 17 == 3) { // refused: oversize, no such channel
        CHECK(!tx.write(chan, msg.data(), kBufSize - 50 + 1));
        CHECK(!tx.write(n_ch, msg.data(), 10));
        CHECK(!tx.write(-1, msg.data(), 10));
      }
      CHECK(tx.write(chan, msg.data(), size));
      tw.write(chan, msg.data(), size);
    }
  };
  const uint32_t flushes[3] = {100, 60, 100}; // buffers 0..99, 100..127 + 0..31 (a wrap), 32..127 + 0..3 (a wrap)
  for (int f = 0; f < 3; f++) {
    queue(flushes[f]);
    if (f == 0) CHECK(!tx.write(0, msg.data(), 10)); // the batch is full
    got.clear();
    const char* e = tx.flush(sink);
    if (e) std::printf("FAIL flush: %s\n", e);
    CHECK(e == nullptr);
    char stage[32];
    std::snprintf(stage, sizeof(stage), "flush %d", f + 1);
    compare(stage, tx, tw, got);
  }
  CHECK(tx.flush(sink) == nullptr); // nothing queued

  { // buildDevice: 50 messages resident on the GPU, packed back to back, one for a channel that does not exist
    const uint32_t n = 50;
    uint64_t* offs;
    uint16_t* lens;
    uint32_t* chans;
    CHECK(hipHostMalloc((void**)&offs, 8 * n, hipHostMallocDefault) == hipSuccess);
    CHECK(hipHostMalloc((void**)&lens, 2 * n, hipHostMallocDefault) == hipSuccess);
    CHECK(hipHostMalloc((void**)&chans, 4 * n, hipHostMallocDefault) == hipSuccess);
    std::vector<uint8_t> pay;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t size = i % 3 == 0 ? sizes[i % 12] : (uint32_t)(rng() % 1999);
      offs[i] = pay.size();
      lens[i] = (uint16_t)size;
      chans[i] = i == 20 ? (uint32_t)n_ch : (uint32_t)(rng() % n_ch);
      for (uint32_t k = 0; k < size; k++) pay.push_back((uint8_t)rng());
    }
    void* d_pay = nullptr;
    CHECK(hipMalloc(&d_pay, pay.size() + 16) == hipSuccess);
    CHECK(hipMemcpy(d_pay, pay.data(), pay.size(), hipMemcpyHostToDevice) == hipSuccess);
    for (uint32_t i = 0; i < n; i++) {
      if (i == 20) tw.skip();
      else tw.write((int)chans[i], pay.data() + offs[i], lens[i]);
    }
    got.clear();
    const char* e = tx.buildDevice(d_pay, pay.size(), offs, lens, chans, n, sink);
    if (e) std::printf("FAIL buildDevice: %s\n", e);
    CHECK(e == nullptr);
    compare("buildDevice", tx, tw, got);
    CHECK(tx.buildDevice(d_pay, pay.size(), offs, lens, chans, 101, sink) != nullptr); // above max_batch
    (void)hipFree(d_pay);
    (void)hipHostFree(offs);
    (void)hipHostFree(lens);
    (void)hipHostFree(chans);
  }

  // the whole ring again in PN_UB_PLAIN mode (two flushes), then through a receiver subscribed to the destinations
  CHECK(tx.setMode(7) != nullptr);
  CHECK(tx.setMode(PN_UB_PLAIN) == nullptr);
  tw.plain = true;
  for (uint32_t count : {100u, 28u}) {
    queue(count);
    got.clear();
    CHECK(tx.flush(sink) == nullptr);
    compare(count == 100 ? "plain flush 1" : "plain flush 2", tx, tw, got);
  }
  {
    GpuUdpReceiver rx;
    const char* e = rx.init(0, kBufSize, GpuUdpSender::kFrameOff, 64);
    if (e) std::printf("FAIL receiver init: %s\n", e);
    CHECK(e == nullptr);
    for (int c = 0; c < n_ch; c++) CHECK(rx.subscribe(kDests[c].dest_ip, kDests[c].dest_port) == c);
    uint32_t slot = 0, delivered = 0;
    e = rx.poll(tx.ring(), kNBuf, [&](int sub, const uint8_t* data, uint16_t len) {
      // every buffer holds a frame, so the calls come one per buffer, in ring order
      CHECK(slot < kNBuf);
      if (slot < kNBuf) {
        CHECK(data == tx.ring() + (size_t)slot * kBufSize + 8 + 42);
        CHECK(sub == tw.slot_chan[slot]);
        CHECK(len == tw.slot_pay[slot].size());
        CHECK(len == tw.slot_pay[slot].size() && std::memcmp(data, tw.slot_pay[slot].data(), len) == 0);
      }
      slot++;
      delivered++;
    });
    if (e) std::printf("FAIL receiver poll: %s\n", e);
    CHECK(e == nullptr);
    CHECK(delivered == kNBuf);
    CHECK(rx.droppedBadIpCsum() == 0 && rx.droppedBadUdpCsum() == 0 && rx.droppedBadLength() == 0);
    std::printf("receiver: %u of %u frames delivered intact\n", delivered, kNBuf);
  }

  std::printf(g_fail ? "FAILED (%d)\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
