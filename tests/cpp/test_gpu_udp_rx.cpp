// GpuUdpReceiver::poll / pollFrom over a pinned host ring of mixed frames vs a sequential loop written here: a host
// filter (the subscription lookup and the checks a NIC makes before it reports EF_EVENT_TYPE_RX), then the
// reference's own read / recvfrom arithmetic (Efvi.h:198-200, 251-255).  Same handler calls, in the same order,
// with the same pointers, lengths and source addresses; the drop counters equal the loop's.  ZeroCopy and Copy.
#include <arpa/inet.h>
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "../../include/pollnet_amd/udp_receiver.hpp"

using pollnet_amd::GpuRx;
using pollnet_amd::GpuUdpReceiver;

namespace {

constexpr uint32_t kStride = 2048, kOff = 2, kBatch = 256, kN = 3 * kBatch + 5;
constexpr uint32_t kAvail = kStride - kOff;

int g_fail = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      g_fail++;                                                  \
    }                                                            \
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
const Dst kSubs[] = {{"239.1.1.1", 12345}, {"239.1.1.2", 12345}, {"239.1.1.1", 12346}, {"10.0.0.9", 53}, {"239.255.0.1", 1}};
const Dst kStrangers[] = {{"239.1.1.1", 12347}, {"239.1.1.3", 12345}, {"10.0.0.8", 53}, {"239.255.0.1", 2}};
constexpr int kNSubs = sizeof(kSubs) / sizeof(kSubs[0]);

void put_frame(uint8_t* slot, std::mt19937& rng, const Dst& d, uint32_t plen, int kind) {
  uint8_t* eth = slot + kOff;
  std::memset(eth, 0, 12);
  eth[6] = 2, eth[11] = 1;
  eth[12] = 0x08, eth[13] = 0x00;
  uint8_t* ip = eth + 14;
  std::memset(ip, 0, 28);
  ip[0] = 0x45;
  uint32_t tot = 28 + plen, ulen = 8 + plen;
  ip[8] = 64, ip[9] = 17;
  const uint32_t src = htonl(0x0A010000u + (rng() & 0xffff));
  std::memcpy(ip + 12, &src, 4);
  inet_pton(AF_INET, d.ip, ip + 16);
  uint8_t* udp = ip + 20;
  const uint16_t sp = htons((uint16_t)(1024 + rng() % 60000)), dp = htons(d.port);
  std::memcpy(udp, &sp, 2);
  std::memcpy(udp + 2, &dp, 2);
  for (uint32_t i = 0; i < plen && 42 + i < kAvail; i++) eth[42 + i] = (uint8_t)rng();
  switch (kind) {
    case 3: ip[6] = 0x20; break;                 // MF
    case 4: ip[9] = 6; break;                    // TCP
    case 5: eth[12] = 0x86, eth[13] = 0xDD; break;
    case 6: ip[0] = 0x46; break;                 // IHL 6
    case 7: ulen = 8 + plen + 2; break;          // ulen above tot_len - 20
    case 8: ulen = kAvail - 33, tot = 20 + ulen; break; // one byte past the slot
    case 9: ulen = 5; break;
    case 10: ip[7] = 9; break;                   // a fragment offset
    default: break;
  }
  ip[2] = tot >> 8, ip[3] = tot & 0xff;
  udp[4] = ulen >> 8, udp[5] = ulen & 0xff;
  uint32_t c = (~ones_sum(ip, 20)) & 0xffff;
  if (kind == 1) c ^= 0x0100; // bad IP checksum
  ip[10] = c >> 8, ip[11] = c & 0xff;
  if (kind != 11 && 34 + ulen <= kAvail) { // kind 11: checksum 0, Efvi's sender
    c = (~udp_sum(eth, ulen)) & 0xffff;
    if (c == 0) c = 0xffff;
    udp[6] = c >> 8, udp[7] = c & 0xff;
  }
  if (kind == 2 && plen) eth[42 + rng() % plen] ^= 0x04; // bad UDP checksum
  if (kind == 12) udp[6] ^= 0x80, ip[10] ^= 0x01;        // both bad
}

void fill_ring(uint8_t* ring, uint32_t seed) {
  std::mt19937 rng(seed);
  for (size_t i = 0; i < (size_t)kN * kStride; i++) ring[i] = (uint8_t)rng(); // garbage after every datagram
  const uint32_t lens[] = {0, 1, 2, 3, 17, 18, 19, 1471, 1472, 100, 701, 1400};
  for (uint32_t i = 0; i < kN; i++) {
    uint8_t* slot = ring + (size_t)i * kStride;
    const uint32_t plen = lens[rng() % 12];
    const uint32_t r = rng() % 100;
    if (r < 40) put_frame(slot, rng, kSubs[rng() % kNSubs], plen, 0);
    else if (r < 50) put_frame(slot, rng, kSubs[rng() % kNSubs], plen, 11);
    else if (r < 65) put_frame(slot, rng, kStrangers[rng() % 4], plen, r & 1 ? 0 : 11);
    else if (r < 95) put_frame(slot, rng, kSubs[rng() % kNSubs], plen ? plen : 4, 1 + (r - 65) % 12);
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

// The sequential loop: a host filter per frame, then the reference's arithmetic on the frames that pass.
Twin sequential(const uint8_t* ring, uint32_t n, const std::map<std::pair<uint32_t, uint16_t>, int>& subs, bool from) {
  Twin t;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* eth = ring + (size_t)i * kStride + kOff;
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
    if (ulen < 8 || tot < 28 || ulen > tot - 20 || 34 + ((ulen + 1) & ~1u) > kAvail) {
      t.drop_len++;
      continue;
    }
    if ((eth[40] | eth[41]) != 0 && udp_sum(eth, ulen) != 0xffff) {
      t.drop_udp++;
      continue;
    }
    // EfviUdpReceiver::read / recvfrom (Efvi.h:198-200, 251-255)
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

void run_mode(GpuRx::Mode mode, const uint8_t* ring) {
  const char* name = mode == GpuRx::Mode::ZeroCopy ? "ZeroCopy" : "Copy";
  GpuUdpReceiver rx;
  const char* e = rx.init(0, kStride, kOff, kBatch, mode);
  if (e) {
    std::printf("FAIL init(%s): %s\n", name, e);
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
  CHECK(subscribe(kSubs[0]) == 0 && subscribe(kSubs[1]) == 1 && subscribe(kSubs[2]) == 2);
  CHECK(rx.subscribe(kSubs[1].ip, kSubs[1].port) == -1); // a pair subscribed already
  CHECK(rx.subscribe("not an address", 1) == -1);
  CHECK(rx.subCount() == 3);

  uint64_t dip = 0, dudp = 0, dlen = 0;
  for (int round = 0; round < 3; round++) {
    if (round == 1) CHECK(subscribe(kSubs[3]) == 3 && subscribe(kSubs[4]) == 4); // after the first poll: next poll
    const bool from = round == 2;
    const uint32_t n = round == 1 ? kBatch + 1 : kN; // one full chunk and a 1-frame chunk
    const Twin want = sequential(ring, n, subs, from);
    std::vector<Call> got;
    if (from)
      e = rx.pollFrom(ring, n, [&](int sub, const uint8_t* d, uint16_t len, const sockaddr_in& src) {
        CHECK(src.sin_family == AF_INET);
        got.push_back(Call{sub, d, len, src.sin_addr.s_addr, src.sin_port});
      });
    else
      e = rx.poll(ring, n, [&](int sub, const uint8_t* d, uint16_t len) { got.push_back(Call{sub, d, len, 0, 0}); });
    if (e) {
      std::printf("FAIL poll(%s, round %d): %s\n", name, round, e);
      g_fail++;
      return;
    }
    dip += want.drop_ip, dudp += want.drop_udp, dlen += want.drop_len;
    CHECK(got.size() == want.calls.size());
    CHECK(got == want.calls);
    CHECK(want.calls.size() > n / 5 && want.calls.size() < n);
    if (n == kN) CHECK(want.drop_ip > 0 && want.drop_udp > 0 && want.drop_len > 0);
    CHECK(rx.droppedBadIpCsum() == dip && rx.droppedBadUdpCsum() == dudp && rx.droppedBadLength() == dlen);
    std::printf("%s round %d: %zu delivered of %u, dropped ip %llu udp %llu len %llu\n", name, round, got.size(), n,
                (unsigned long long)want.drop_ip, (unsigned long long)want.drop_udp, (unsigned long long)want.drop_len);
  }
  CHECK(rx.poll(ring, 0, [](int, const uint8_t*, uint16_t) {}) == nullptr);
}

} // namespace

int main() {
  int ndev = 0;
  if (pn_device_count(&ndev) || ndev == 0) {
    std::printf("no GPU\n");
    return 2;
  }
  uint8_t* ring = nullptr;
  if (hipHostMalloc((void**)&ring, (size_t)kN * kStride, hipHostMallocDefault) != hipSuccess) {
    std::printf("hipHostMalloc failed\n");
    return 1;
  }
  fill_ring(ring, 20241);
  run_mode(GpuRx::Mode::ZeroCopy, ring);
  run_mode(GpuRx::Mode::Copy, ring);
  {
    GpuUdpReceiver rx; // an unpinned ring is refused in ZeroCopy mode, before anything is launched
    std::vector<uint8_t> plain((size_t)4 * kStride);
    CHECK(rx.init(0, kStride, kOff, 4, GpuRx::Mode::ZeroCopy) == nullptr);
    CHECK(rx.subscribe("239.1.1.1", 1) == 0);
    CHECK(rx.poll(plain.data(), 4, [](int, const uint8_t*, uint16_t) {}) != nullptr);
  }
  (void)hipHostFree(ring);
  std::printf(g_fail ? "FAILED (%d)\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
