// GpuUdpReceiver::gatherBySub / gatherBySubIndexed (include/pollnet_amd/udp_receiver.hpp) against the (sub, data, len)
// calls that poll / pollIndexed make on the same ring, bucketed per subscription in call order: subscription s's
// messages are messages [sub_first[s], sub_first[s+1]) and bytes [sub_bytes[s], sub_bytes[s+1]) of the device buffer,
// each 16-byte aligned and zero-padded, src_index naming the frame the handler's pointer was in.  The ring is built
// by a GpuUdpSender in PN_UB_CSUM mode, then damaged here and there (a payload bit, a header bit) and holds a
// destination nobody subscribed to, so that not every frame is delivered; one subscription receives nothing.  Run
// from pinned and from device slots.  Then a relay without the host in the data path: gatherBySub ->
// GpuUdpSender::buildDevice with the grouped arrays (subs as channels) -> a second receiver subscribed to the relay's
// destinations: every payload arrives intact, one subscription after the other, each in order.
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

constexpr uint32_t kNBuf = 128, kBufSize = 2048, kOff = GpuUdpSender::kFrameOff;
const uint8_t kLocalMac[6] = {0x00, 0x0f, 0x53, 0x10, 0x20, 0x30};
struct Dest {
  const char* ip;
  uint16_t port;
};
const Dest kDests[] = {{"239.1.2.3", 20001}, {"239.1.2.4", 20001}, {"239.200.130.9", 20002}, {"239.9.9.9", 20003},
                       {"239.77.0.1", 20004}}; // the last one: nobody subscribes
const Dest kRelay[] = {{"239.50.0.1", 30001}, {"239.50.0.2", 30001}, {"239.50.0.3", 30002}, {"239.50.0.4", 30003},
                       {"239.50.0.5", 30004}};
const Dest kQuiet = {"239.66.0.1", 20009}; // subscribed (index 2 of 5), never sent to
constexpr int kSubs = 5;
// the receiver's subscription for sender channel c (the quiet one sits in the middle); -1: nobody subscribes
int sub_of_channel(int c) { return c < 2 ? c : c < 4 ? c + 1 : -1; }

struct Call {
  int sub;
  const uint8_t* data;
  uint16_t len;
};

template <class T>
std::vector<T> to_host(const T* dev, size_t n) {
  std::vector<T> v(n);
  if (n) CHECK(hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  return v;
}

// The handler calls bucketed per subscription, in call order: what the grouped batch must hold.
std::vector<Call> bucketed(const std::vector<Call>& calls, std::vector<uint32_t>* first) {
  std::vector<Call> out;
  first->assign(kSubs + 1, 0);
  for (int s = 0; s < kSubs; s++) {
    (*first)[s] = (uint32_t)out.size();
    for (const Call& c : calls)
      if (c.sub == s) out.push_back(c);
  }
  (*first)[kSubs] = (uint32_t)out.size();
  return out;
}

// The grouped batch against the handler calls; `ring` is where the handler's pointers point into (host), eth_of(i)
// frame i's Ethernet header in it.
template <class EthOf>
void compare(const char* stage, const GpuUdpReceiver::GatheredBySub& g, const std::vector<Call>& polled, EthOf&& eth_of) {
  const int before = g_fail;
  std::vector<uint32_t> want_first;
  const std::vector<Call> calls = bucketed(polled, &want_first);
  CHECK(g.n_msgs == calls.size());
  CHECK(g.n_fit == g.n_msgs);
  const uint32_t n = g.n_msgs < calls.size() ? g.n_msgs : (uint32_t)calls.size();
  const auto offs = to_host(g.offs, n);
  const auto lens = to_host(g.lens, n);
  const auto subs = to_host(g.subs, n);
  const auto src = to_host(g.src_index, n);
  const auto pay = to_host(g.payloads, (size_t)g.n_bytes);
  const auto first = to_host(g.sub_first, kSubs + 1);
  const auto sbytes = to_host(g.sub_bytes, kSubs + 1);
  uint64_t at = 0;
  int s = 0;
  for (uint32_t j = 0; j < n; j++) {
    const Call& c = calls[j];
    for (; s <= c.sub; s++) CHECK(first[s] == want_first[s] && sbytes[s] == at); // this and the empty ones before it
    CHECK(offs[j] == at && offs[j] % 16 == 0);
    CHECK(lens[j] == c.len && (int)subs[j] == c.sub);
    CHECK(eth_of(src[j]) + 42 == c.data);
    const uint64_t end = at + ((c.len + 15u) & ~15u);
    CHECK(end <= pay.size());
    if (end > pay.size()) break;
    CHECK(std::memcmp(pay.data() + at, c.data, c.len) == 0);
    for (uint64_t k = at + c.len; k < end; k++) CHECK(pay[k] == 0);
    at = end;
  }
  for (; s <= kSubs; s++) CHECK(first[s] == want_first[s] && sbytes[s] == at);
  CHECK(first[2] == first[3] && sbytes[2] == sbytes[3]); // the quiet subscription owns nothing
  CHECK(g.n_bytes == at);
  std::printf("%s: %u messages, %llu bytes%s\n", stage, g.n_msgs, (unsigned long long)g.n_bytes,
              g_fail == before ? "" : "  (FAILED)");
}

} // namespace

int main() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::printf("no GPU\n");
    return 2;
  }
  // ---- a ring of 128 datagrams for 5 destinations, with their UDP checksums ----
  GpuUdpSender tx;
  if (const char* e = tx.init(0, kNBuf)) {
    std::printf("FAIL init: %s\n", e);
    return 1;
  }
  for (int c = 0; c < 5; c++) CHECK(tx.addChannel("10.20.30.40", 40000 + c, kLocalMac, kDests[c].ip, kDests[c].port, nullptr) == c);
  CHECK(tx.setMode(PN_UB_CSUM) == nullptr);
  std::mt19937 rng(1717);
  std::vector<uint8_t> msg(2048);
  const uint32_t sizes[] = {0, 1, 15, 16, 17, 64, 127, 128, 129, 1024, 1472, 1998};
  for (uint32_t k = 0; k < kNBuf; k++) {
    const uint32_t size = k % 3 == 2 ? (uint32_t)(rng() % 1999) : sizes[(k / 3) % 12];
    for (uint32_t i = 0; i < size; i++) msg[i] = (uint8_t)(1 + rng() % 255);
    CHECK(tx.write((int)(rng() % 5), msg.data(), size));
  }
  CHECK(tx.flush([](const uint8_t*, uint32_t, uint32_t) {}) == nullptr);
  uint8_t* ring = tx.ring();
  for (uint32_t b = 5; b < kNBuf; b += 11) { // damage: a payload bit (or the length field of an empty datagram), a header bit
    uint8_t* eth = ring + (size_t)b * kBufSize + kOff;
    const uint32_t len = (uint32_t)((eth[38] << 8) | eth[39]) - 8;
    if (b % 2) eth[len ? 42 + len / 2 : 39] ^= 0x04;
    else eth[22] ^= 0x01; // ttl: the IPv4 checksum fails
  }

  GpuUdpReceiver rx;
  const char* e = rx.init(0, kBufSize, kOff, kNBuf);
  if (e) std::printf("FAIL receiver init: %s\n", e);
  CHECK(e == nullptr);
  for (int c = 0; c < 4; c++) {
    if (c == 2) CHECK(rx.subscribe(kQuiet.ip, kQuiet.port) == 2);
    CHECK(rx.subscribe(kDests[c].ip, kDests[c].port) == sub_of_channel(c));
  }
  CHECK(rx.subCount() == kSubs);
  GpuUdpReceiver::GatheredBySub g{};

  // ---- gatherBySub vs poll, slots in pinned memory ----
  std::vector<Call> calls;
  auto handler = [&](int sub, const uint8_t* data, uint16_t len) { calls.push_back({sub, data, len}); };
  CHECK(rx.poll(ring, kNBuf, handler) == nullptr);
  const uint64_t d_ip = rx.droppedBadIpCsum(), d_udp = rx.droppedBadUdpCsum(), d_len = rx.droppedBadLength();
  CHECK(calls.size() > 60 && calls.size() < kNBuf && d_ip > 0 && d_udp > 0);
  e = rx.gatherBySub(ring, kNBuf, &g);
  if (e) std::printf("FAIL gatherBySub: %s\n", e);
  CHECK(e == nullptr);
  auto slot_eth = [&](uint32_t i) { return (const uint8_t*)ring + (size_t)i * kBufSize + kOff; };
  compare("gatherBySub (pinned slots)", g, calls, slot_eth);
  CHECK(rx.droppedBadIpCsum() == d_ip && rx.droppedBadUdpCsum() == d_udp && rx.droppedBadLength() == d_len);
  CHECK(rx.gatherBySub(ring, kNBuf + 1, &g) != nullptr); // above max_batch
  CHECK(rx.gatherBySub(ring, kNBuf, nullptr) != nullptr);
  CHECK(rx.gatherBySub(ring, 0, &g) == nullptr && g.n_msgs == 0 && g.n_bytes == 0 && g.sub_first == nullptr);
  { // gather keeps its behaviour beside it: the same messages in arrival order
    GpuUdpReceiver::Gathered a{};
    CHECK(rx.gather(ring, kNBuf, &a) == nullptr && a.n_msgs == calls.size() && a.n_fit == a.n_msgs);
    const auto a_src = to_host(a.src_index, a.n_msgs);
    for (uint32_t j = 0; j < a.n_msgs && j < calls.size(); j++) CHECK(slot_eth(a_src[j]) + 42 == calls[j].data);
  }

  // ---- the same slots in device memory; a batch that is not the whole ring ----
  uint8_t* d_ring = nullptr;
  CHECK(hipMalloc((void**)&d_ring, (size_t)kNBuf * kBufSize) == hipSuccess);
  CHECK(hipMemcpy(d_ring, ring, (size_t)kNBuf * kBufSize, hipMemcpyHostToDevice) == hipSuccess);
  e = rx.gatherBySub(d_ring, kNBuf, &g);
  CHECK(e == nullptr);
  compare("gatherBySub (device slots)", g, calls, slot_eth);
  {
    std::vector<Call> part;
    CHECK(rx.poll(ring + (size_t)7 * kBufSize, 70, [&](int sub, const uint8_t* data, uint16_t len) { part.push_back({sub, data, len}); }) == nullptr);
    e = rx.gatherBySub(d_ring + (size_t)7 * kBufSize, 70, &g);
    CHECK(e == nullptr);
    compare("gatherBySub (70 slots from slot 7)", g, part, [&](uint32_t i) { return slot_eth(7 + i); });
  }

  // ---- gatherBySubIndexed vs pollIndexed: an event run that wraps, repeats and skips, one offset outside the class ----
  {
    std::vector<uint64_t> offsets;
    for (uint32_t i = 100; offsets.size() < 120; i++) {
      if (i % 7 == 3) continue;
      offsets.push_back((uint64_t)(i % kNBuf) * kBufSize + kOff);
      if (i % 13 == 0) offsets.push_back(offsets.back());
    }
    offsets[50] += 2;
    std::vector<Call> ic;
    const uint64_t len_before = rx.droppedBadLength();
    CHECK(rx.pollIndexed(ring, offsets.data(), (uint32_t)offsets.size(), kOff, kBufSize - kOff,
                         [&](int sub, const uint8_t* data, uint16_t len) { ic.push_back({sub, data, len}); }) == nullptr);
    CHECK(rx.droppedBadLength() > len_before);
    const uint64_t i_ip = rx.droppedBadIpCsum(), i_udp = rx.droppedBadUdpCsum(), i_len = rx.droppedBadLength();
    auto off_eth = [&](uint32_t i) { return (const uint8_t*)ring + offsets[i]; };
    e = rx.gatherBySubIndexed(ring, offsets.data(), (uint32_t)offsets.size(), kOff, kBufSize - kOff, &g);
    if (e) std::printf("FAIL gatherBySubIndexed: %s\n", e);
    CHECK(e == nullptr);
    compare("gatherBySubIndexed (pinned ring)", g, ic, off_eth);
    e = rx.gatherBySubIndexed(d_ring, offsets.data(), (uint32_t)offsets.size(), kOff, kBufSize - kOff, &g);
    CHECK(e == nullptr);
    compare("gatherBySubIndexed (device ring)", g, ic, off_eth);
    CHECK(rx.droppedBadIpCsum() == i_ip && rx.droppedBadUdpCsum() == i_udp && rx.droppedBadLength() == i_len);
    CHECK(rx.gatherBySubIndexed(ring, offsets.data(), kNBuf + 1, kOff, kBufSize - kOff, &g) != nullptr);
    CHECK(rx.gatherBySubIndexed(ring, nullptr, 5, kOff, kBufSize - kOff, &g) != nullptr);
  }

  // ---- relay: gatherBySub -> buildDevice (subs as channels) -> a second receiver ----
  {
    e = rx.gatherBySub(d_ring, kNBuf, &g);
    CHECK(e == nullptr && g.n_msgs == calls.size());
    std::vector<uint32_t> want_first;
    const std::vector<Call> grouped = bucketed(calls, &want_first);
    GpuUdpSender relay;
    CHECK(relay.init(0, kNBuf) == nullptr);
    for (int c = 0; c < kSubs; c++)
      CHECK(relay.addChannel("10.99.0.1", 50000 + c, kLocalMac, kRelay[c].ip, kRelay[c].port, nullptr) == c);
    CHECK(relay.setMode(PN_UB_CSUM) == nullptr);
    uint32_t sunk = 0;
    e = relay.buildDevice(g.payloads, g.n_bytes, g.offs, g.lens, g.subs, g.n_msgs,
                          [&](const uint8_t*, uint32_t, uint32_t) { sunk++; });
    if (e) std::printf("FAIL relay buildDevice: %s\n", e);
    CHECK(e == nullptr && sunk == g.n_msgs);
    GpuUdpReceiver rx2;
    CHECK(rx2.init(0, kBufSize, kOff, 64) == nullptr);
    for (int c = 0; c < kSubs; c++) CHECK(rx2.subscribe(kRelay[c].ip, kRelay[c].port) == c);
    uint32_t j = 0;
    int last_sub = 0;
    e = rx2.poll(relay.ring(), g.n_msgs, [&](int sub, const uint8_t* data, uint16_t len) {
      CHECK(j < grouped.size());
      if (j < grouped.size()) {
        CHECK(sub == grouped[j].sub && len == grouped[j].len);
        CHECK(len == grouped[j].len && std::memcmp(data, grouped[j].data, len) == 0);
        CHECK(data == relay.ring() + (size_t)j * kBufSize + kOff + 42);
      }
      CHECK(sub >= last_sub); // one channel at a time
      last_sub = sub;
      j++;
    });
    CHECK(e == nullptr && j == grouped.size());
    CHECK(rx2.droppedBadIpCsum() == 0 && rx2.droppedBadUdpCsum() == 0 && rx2.droppedBadLength() == 0);
    std::printf("relay: %u of %zu payloads arrived intact, grouped by channel\n", j, grouped.size());
  }
  (void)hipFree(d_ring);

  std::printf(g_fail ? "FAILED (%d)\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
