// EfviUdpRingLayout (include/pollnet_amd/rx_ring.hpp) against the reference's own arithmetic, restated here from
// Efvi.h:115-116, 140, 194-200: N_BUF = 511 buffers of PKT_BUF_SIZE = 2048 B, and EfviUdpReceiver::read takes the
// payload from pkt_bufs + id * PKT_BUF_SIZE + udp_prefix_len, udp_prefix_len = 64 + prefix + 14 + 20 + 8.  Host only.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/pollnet_amd/rx_ring.hpp"

using pollnet_amd::EfviRingLayout;
using pollnet_amd::EfviUdpRingLayout;

namespace {
int g_fail = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                \
    }                                                          \
  } while (0)
} // namespace

int main() {
  static_assert(EfviUdpRingLayout::kBufCnt == 511 && EfviUdpRingLayout::kPktBufSize == 2048, "Efvi.h:115-116");
  for (uint32_t prefix = 0; prefix <= 64; prefix++) {
    EfviUdpRingLayout L;
    L.prefix_len = prefix;
    const uint32_t udp_prefix_len = 64 + prefix + 14 + 20 + 8; // Efvi.h:140
    CHECK(L.frame_off() == 64 + prefix);
    CHECK(L.frame_off() + 42 == udp_prefix_len);
    CHECK(L.eth_mod16() == prefix % 16 && L.eth_mod16() == L.frame_off() % 16);
    CHECK(L.avail() == 2048 - 64 - prefix);
    CHECK(L.frame_off() + L.avail() == EfviUdpRingLayout::kPktBufSize); // a frame's bytes end with its buffer
    CHECK(L.ring_bytes() == 511u * 2048u);
    // an event run that wraps the ring, reposts ids and skips discarded ones
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < 1300; i++)
      if (i % 7 != 3) ids.push_back(i % 511);
    ids.push_back(510), ids.push_back(0), ids.push_back(510);
    std::vector<uint64_t> offs(ids.size(), ~0ull);
    L.offsets(ids.data(), (uint32_t)ids.size(), offs.data());
    for (size_t i = 0; i < ids.size(); i++) {
      CHECK(offs[i] == (uint64_t)ids[i] * 2048 + udp_prefix_len - 42); // the payload read()'s pointer is 42 B on
      CHECK(offs[i] == L.offset(ids[i]));
      CHECK(offs[i] % 16 == L.eth_mod16());
      CHECK(offs[i] + L.avail() <= L.ring_bytes());
      CHECK(offs[i] + L.avail() == ((uint64_t)ids[i] + 1) * 2048);
    }
  }
  {
    EfviUdpRingLayout L; // the last buffer's frame ends with the ring
    L.prefix_len = 2;
    CHECK(L.offset(510) + L.avail() == L.ring_bytes());
    EfviRingLayout T; // efvitcp's ring is another layout: a 10-B RecvBuf header
    T.prefix_len = 2;
    CHECK(T.frame_off() == 12 && L.frame_off() == 66);
  }
  std::printf(g_fail ? "FAILED (%d)\n" : "PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
