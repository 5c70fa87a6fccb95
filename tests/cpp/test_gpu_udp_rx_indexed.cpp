// GpuUdpReceiver::pollIndexed / pollFromIndexed over pollnet's ef_vi UDP ring (EfviUdpRingLayout: 511 buffers of
// 2048 B, the frame at 64 + prefix_len) driven by an RX-event run that wraps the ring, reposts ids and skips
// discarded buffers, vs a sequential loop written here: a host filter (the subscription lookup and the checks a NIC
// makes before it reports EF_EVENT_TYPE_RX), then the reference's own read / recvfrom arithmetic on the buffer the
// event names (Efvi.h:194-200, 251-255).  Same handler calls, in the same order, with the same pointers, lengths and
// source addresses; the drop counters equal the loop's, an offset outside the alignment class counting as a bad
// length; two rounds, max_batch smaller than the run.  Copy mode returns the error.
#include <arpa/inet.h>
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "../../include/pollnet_amd/rx_ring.hpp"
#include "../../include/pollnet_amd/udp_receiver.hpp"

using pollnet_amd::EfviUdpRingLayout;
using pollnet_amd::GpuRx;
using pollnet_amd::GpuUdpReceiver;

namespace {

constexpr uint32_t kBatch = 256, kEvents = 1300;

int g_fail = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                \
    }                                                          \
  } while (0)

// RFC 1071 over big-endian words, an odd tail zero-padded, folded
uint32_t ones_sum(const uint8_t* p, size_t n, uint32_t s = 0) {
  for (size_t i = 0; i + 1 < n; i += 2) s += (uint32_t)p[i] << 8 | p[i + 1];
  if (n & 1) s += (uint32_t)p[n - 1] << 8;
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return s;
}

uint32_t udp_sum(const uint8_t* eth, uint32_t ulen) { // pseudo-header + ulen bytes at eth + 34
  uint8_t ph[12];
  std::memcpy(ph, eth + 26, 8);
  ph[8] = 0, ph[9] = 17;
  std::memcpy(ph + 10, eth + 38, 2);
  return ones_sum(eth + 34, ulen, ones_sum(ph, 12));
}

struct Dst {
  const char* ip;
  uint16_t port;
};
const Dst kSubs[] = {{"239.2.1.1", 31001}, {"239.2.1.2", 31001}, {"239.2.1.1", 31002}, {"10.0.0.7", 5353}};
const Dst kStrangers[] = {{"239.2.1.1", 31003}, {"239.2.1.3", 31001}, {"10.0.0.6", 5353}};
constexpr int kNSubs = sizeof(kSubs) / sizeof(kSubs[0]);

// kind 0 good, 1 bad IP checksum, 2 bad UDP checksum, 3 MF, 4 TCP, 5 ulen above tot_len - 20, 6 one byte past the
// buffer, 7 checksum 0
void put_frame(uint8_t* eth, uint32_t avail, std::mt19937& rng, const Dst& d, uint32_t plen, int kind) {
  std::memset(eth, 0, 42);
  eth[6] = 2, eth[11] = 1, eth[12] = 0x08;
  uint8_t* ip = eth + 14;
  ip[0] = 0x45, ip[8] = 64, ip[9] = 17;
  uint32_t tot = 28 + plen, ulen = 8 + plen;
  const uint32_t src = htonl(0x0A020000u + (rng() & 0xffff));
  std::memcpy(ip + 12, &src, 4);
  inet_pton(AF_INET, d.ip, ip + 16);
  uint8_t* udp = ip + 20;
  const uint16_t sp = htons((uint16_t)(1024 + rng() % 60000)), dp = htons(d.port);
  std::memcpy(udp, &sp, 2);
  std::memcpy(udp + 2, &dp, 2);
  for (uint32_t i = 0; i < plen && 42 + i < avail; i++) eth[42 + i] = (uint8_t)rng();
  if (kind == 3) ip[6] = 0x20;
  if (kind == 4) ip[9] = 6;
  if (kind == 5) ulen += 2;
  if (kind == 6) ulen = avail - 33, tot = 20 + ulen;
  ip[2] = tot >> 8, ip[3] = tot & 0xff;
  udp[4] = ulen >> 8, udp[5] = ulen & 0xff;
  uint32_t c = (~ones_sum(ip, 20)) & 0xffff;
  if (kind == 1) c ^= 0x0100;
  ip[10] = c >> 8, ip[11] = c & 0xff;
  if (kind != 7 && 34 + ulen <= avail) {
    c = (~udp_sum(eth, ulen)) & 0xffff;
    if (c == 0) c = 0xffff;
    udp[6] = c >> 8, udp[7] = c & 0xff;
  }
  if (kind == 2 && plen) eth[42 + rng() % plen] ^= 0x04;
}

void fill_ring(uint8_t* ring, const EfviUdpRingLayout& L, uint32_t seed) {
  std::mt19937 rng(seed);
  for (size_t i = 0; i < L.ring_bytes(); i++) ring[i] = (uint8_t)rng(); // garbage after every datagram
  const uint32_t lens[] = {0, 1, 2, 3, 17, 18, 19, 1471, 1472, 100, 701, 1400};
  for (uint32_t id = 0; id < EfviUdpRingLayout::kBufCnt; id++) {
    uint8_t* eth = ring + L.offset(id);
    const uint32_t plen = lens[rng() % 12], r = rng() % 100;
    if (r < 40) put_frame(eth, L.avail(), rng, kSubs[rng() % kNSubs], plen, 0);
    else if (r < 50) put_frame(eth, L.avail(), rng, kSubs[rng() % kNSubs], plen, 7);
    else if (r < 65) put_frame(eth, L.avail(), rng, kStrangers[rng() % 3], plen, r & 1 ? 0 : 7);
    else if (r < 95) put_frame(eth, L.avail(), rng, kSubs[rng() % kNSubs], plen ? plen : 4, 1 + (r - 65) % 6);
    // else: random bytes
  }
}

struct Call {
  int sub;
  const uint8_t* data;
  uint16_t len;
  uint32_t src_ip;
  uint16_t src_port;
  bool operator==(const Call& o) const {
    return sub == o.sub && data == o.data && len == o.len && src_ip == o.src_ip && src_port == o.src_port;
  }
};

struct Twin {
  std::vector<Call> calls;
  uint64_t drop_ip = 0, drop_udp = 0, drop_len = 0;
};

// The sequential loop, event by event: the buffer the event names, a host filter, the reference's arithmetic.
Twin sequential(const uint8_t* ring, const std::vector<uint64_t>& offs, uint32_t eth_mod16, uint32_t avail,
                const std::map<std::pair<uint32_t, uint16_t>, int>& subs, bool from) {
  Twin t;
  for (uint64_t o : offs) {
    if (o % 16 != eth_mod16) { // not a frame of this ring's layout: never read
      t.drop_len++;
      continue;
    }
    const uint8_t* eth = ring + o;
    if (eth[12] != 0x08 || eth[13] != 0x00 || eth[14] != 0x45 || eth[23] != 17) continue;
    if (((eth[20] & 0x3f) | eth[21]) != 0) continue; // MF or a fragment offset
    uint32_t dip;
    uint16_t dport;
    std::memcpy(&dip, eth + 30, 4);
    std::memcpy(&dport, eth + 36, 2);
    auto it = subs.find({dip, dport});
    if (it == subs.end()) continue;
    const uint32_t tot = (uint32_t)eth[16] << 8 | eth[17], ulen = (uint32_t)eth[38] << 8 | eth[39];
    if (ones_sum(eth + 14, 20) != 0xffff) {
      t.drop_ip++;
      continue;
    }
    if (ulen < 8 || tot < 28 || ulen > tot - 20 || 34 + ((ulen + 1) & ~1u) > avail) {
      t.drop_len++;
      continue;
    }
    if ((eth[40] | eth[41]) != 0 && udp_sum(eth, ulen) != 0xffff) {
      t.drop_udp++;
      continue;
    }
    // EfviUdpReceiver::read / recvfrom (Efvi.h:198-200, 251-255): data = pkt_buf + udp_prefix_len
    const uint8_t* data = eth + 42;
    uint16_t be_len;
    std::memcpy(&be_len, data - 4, 2);
    const uint16_t len = ntohs(be_len) - 8;
    Call c{it->second, data, len, 0, 0};
    if (from) {
      std::memcpy(&c.src_ip, data - 16, 4);
      std::memcpy(&c.src_port, data - 8, 2);
    }
    t.calls.push_back(c);
  }
  return t;
}

// An RX-event run: ids in ring order over more than two laps, every 7th buffer discarded (no event), a buffer
// reposted and named again at once now and then.
std::vector<uint32_t> event_ids(uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> ids;
  for (uint32_t i = 0; ids.size() < kEvents; i++) {
    const uint32_t id = i % EfviUdpRingLayout::kBufCnt;
    if (i % 7 == 3) continue;
    ids.push_back(id);
    if (rng() % 40 == 0 && ids.size() < kEvents) ids.push_back(id);
  }
  return ids;
}

void run_prefix(uint32_t prefix, uint8_t* ring) {
  EfviUdpRingLayout L;
  L.prefix_len = prefix;
  fill_ring(ring, L, 7000 + prefix);
  GpuUdpReceiver rx;
  // the strided layout of init plays no part in indexed polls
  const char* e = rx.init(0, 2048, 2, kBatch, GpuRx::Mode::ZeroCopy);
  if (e) {
    std::printf("FAIL init: %s\n", e);
    g_fail++;
    return;
  }
  std::map<std::pair<uint32_t, uint16_t>, int> subs;
  auto subscribe = [&](const Dst& d) {
    const int id = rx.subscribe(d.ip, d.port);
    uint32_t ip;
    inet_pton(AF_INET, d.ip, &ip);
    subs[{ip, htons(d.port)}] = id;
    return id;
  };
  CHECK(subscribe(kSubs[0]) == 0 && subscribe(kSubs[1]) == 1);

  uint64_t dip = 0, dudp = 0, dlen = 0;
  for (int round = 0; round < 2; round++) {
    if (round == 1) CHECK(subscribe(kSubs[2]) == 2 && subscribe(kSubs[3]) == 3);
    const bool from = round == 1;
    const std::vector<uint32_t> ids = event_ids(100 * prefix + round);
    std::vector<uint64_t> offs(ids.size());
    L.offsets(ids.data(), (uint32_t)ids.size(), offs.data());
    uint32_t strays = 0;
    if (round == 1) // a few offsets that are no frame of this layout, one of them a chunk's first
      for (size_t i : {(size_t)5, (size_t)kBatch, (size_t)2 * kBatch - 1, offs.size() - 1}) offs[i] += 2, strays++;
    const uint32_t n = (uint32_t)offs.size();
    CHECK(n == kEvents && n > 2 * EfviUdpRingLayout::kBufCnt && n % kBatch != 0);
    const Twin want = sequential(ring, offs, L.eth_mod16(), L.avail(), subs, from);
    std::vector<Call> got;
    if (from)
      e = rx.pollFromIndexed(ring, offs.data(), n, L.eth_mod16(), L.avail(),
                             [&](int sub, const uint8_t* d, uint16_t len, const sockaddr_in& src) {
                               CHECK(src.sin_family == AF_INET);
                               got.push_back(Call{sub, d, len, src.sin_addr.s_addr, src.sin_port});
                             });
    else
      e = rx.pollIndexed(ring, offs.data(), n, L.eth_mod16(), L.avail(),
                         [&](int sub, const uint8_t* d, uint16_t len) { got.push_back(Call{sub, d, len, 0, 0}); });
    if (e) {
      std::printf("FAIL poll(prefix %u, round %d): %s\n", prefix, round, e);
      g_fail++;
      return;
    }
    dip += want.drop_ip, dudp += want.drop_udp, dlen += want.drop_len;
    CHECK(got.size() == want.calls.size());
    CHECK(got == want.calls);
    CHECK(want.calls.size() > n / 8 && want.calls.size() < n);
    CHECK(want.drop_ip > 0 && want.drop_udp > 0 && want.drop_len > strays);
    CHECK(rx.droppedBadIpCsum() == dip && rx.droppedBadUdpCsum() == dudp && rx.droppedBadLength() == dlen);
    std::printf("prefix %u round %d: %zu delivered of %u events, dropped ip %llu udp %llu len %llu\n", prefix, round,
                got.size(), n, (unsigned long long)want.drop_ip, (unsigned long long)want.drop_udp,
                (unsigned long long)want.drop_len);
  }
  const uint64_t none = 0;
  CHECK(rx.pollIndexed(ring, &none, 0, L.eth_mod16(), L.avail(), [](int, const uint8_t*, uint16_t) {}) == nullptr);
}

} // namespace

int main() {
  int ndev = 0;
  if (pn_device_count(&ndev) || ndev == 0) {
    std::printf("no GPU\n");
    return 2;
  }
  EfviUdpRingLayout L;
  uint8_t* ring = nullptr;
  if (hipHostMalloc((void**)&ring, L.ring_bytes(), hipHostMallocDefault) != hipSuccess) {
    std::printf("hipHostMalloc failed\n");
    return 1;
  }
  for (uint32_t prefix : {0u, 2u, 14u}) run_prefix(prefix, ring);
  {
    GpuUdpReceiver rx; // Copy mode has no indexed path: the error, before anything is launched
    const uint64_t off = L.offset(0);
    int calls = 0;
    CHECK(rx.init(0, 2048, 2, 4, GpuRx::Mode::Copy) == nullptr);
    CHECK(rx.subscribe("239.2.1.1", 31001) == 0);
    const char* e = rx.pollIndexed(ring, &off, 1, L.eth_mod16(), L.avail(), [&](int, const uint8_t*, uint16_t) { calls++; });
    CHECK(e != nullptr && std::strstr(e, "ZeroCopy") != nullptr && calls == 0);
    e = rx.pollFromIndexed(ring, &off, 1, L.eth_mod16(), L.avail(),
                           [&](int, const uint8_t*, uint16_t, const sockaddr_in&) { calls++; });
    CHECK(e != nullptr && std::strstr(e, "ZeroCopy") != nullptr && calls == 0);
    std::printf("Copy mode: %s\n", e ? e : "(no error)");
  }
  {
    GpuUdpReceiver rx; // an unpinned ring is refused, before anything is launched
    std::vector<uint8_t> plain(4 * 2048);
    const uint64_t off = 64;
    CHECK(rx.init(0, 2048, 2, 4, GpuRx::Mode::ZeroCopy) == nullptr);
    CHECK(rx.subscribe("239.2.1.1", 31001) == 0);
    CHECK(rx.pollIndexed(plain.data(), &off, 1, 0, 1984, [](int, const uint8_t*, uint16_t) {}) != nullptr);
  }
  (void)hipHostFree(ring);
  std::printf(g_fail ? "FAILED (%d)\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
