// udp_sender_template (GpuUdpSender::addChannel's header) against EfviUdpSender::init's 42 bytes written out by
// hand (Efvi.h:344-378, 597-644): one unicast and one multicast destination.  Host only.
#include <cstdio>
#include <cstring>

#include "../../include/pollnet_amd/udp_sender.hpp"

static int fails = 0;

static void expect(const char* what, const pn_udp_channel& c, const uint8_t (&want)[42]) {
  if (std::memcmp(c.hdr, want, 42) != 0) {
    fails++;
    std::printf("FAIL %s:\n  got ", what);
    for (int i = 0; i < 42; i++) std::printf("%02x", c.hdr[i]);
    std::printf("\n  want ");
    for (int i = 0; i < 42; i++) std::printf("%02x", want[i]);
    std::printf("\n");
  }
  for (uint8_t p : c._pad)
    if (p) {
      fails++;
      std::printf("FAIL %s: non-zero _pad\n", what);
    }
}

int main() {
  using pollnet_amd::udp_sender_template;
  const uint8_t lmac[6] = {0x00, 0x0f, 0x53, 0x0a, 0x0b, 0x0c};
  const uint8_t dmac[6] = {0x3c, 0xfd, 0xfe, 0x01, 0x02, 0x03};
  pn_udp_channel c;
  std::memset(&c, 0xEE, sizeof(c));

  // unicast 192.168.10.5:1000 -> 192.168.10.77:31001, the MAC as given
  const uint8_t uni[42] = {0x3c, 0xfd, 0xfe, 0x01, 0x02, 0x03, 0x00, 0x0f, 0x53, 0x0a, 0x0b, 0x0c, 0x08, 0x00, // eth
                           0x45, 0x00, 0x00, 0x00, 0x00, 0x00, 0x40, 0x00, 0x40, 0x11, 0x00, 0x00,             // ip
                           192,  168,  10,   5,    192,  168,  10,   77,                                      // addresses
                           0x03, 0xe8, 0x79, 0x19, 0x00, 0x08, 0x00, 0x00};                                   // udp
  if (!udp_sender_template(&c, "192.168.10.5", 1000, lmac, "192.168.10.77", 31001, dmac)) {
    fails++;
    std::printf("FAIL unicast refused\n");
  }
  expect("unicast", c, uni);

  // multicast 10.1.2.3:20000 -> 239.129.2.3:20001: 01:00:5e + the low 23 bits (129 & 0x7f = 1), dest_mac ignored / null
  const uint8_t mc[42] = {0x01, 0x00, 0x5e, 0x01, 0x02, 0x03, 0x00, 0x0f, 0x53, 0x0a, 0x0b, 0x0c, 0x08, 0x00,
                          0x45, 0x00, 0x00, 0x00, 0x00, 0x00, 0x40, 0x00, 0x40, 0x11, 0x00, 0x00,
                          10,   1,    2,    3,    239,  129,  2,    3,
                          0x4e, 0x20, 0x4e, 0x21, 0x00, 0x08, 0x00, 0x00};
  std::memset(&c, 0xEE, sizeof(c));
  if (!udp_sender_template(&c, "10.1.2.3", 20000, lmac, "239.129.2.3", 20001, nullptr)) {
    fails++;
    std::printf("FAIL multicast refused\n");
  }
  expect("multicast (null mac)", c, mc);
  std::memset(&c, 0xEE, sizeof(c));
  (void)udp_sender_template(&c, "10.1.2.3", 20000, lmac, "239.129.2.3", 20001, dmac);
  expect("multicast (mac given)", c, mc);

  // no ARP: a unicast destination without a MAC, and bad addresses, are refused
  if (udp_sender_template(&c, "10.1.2.3", 1, lmac, "10.1.2.4", 2, nullptr)) fails++, std::printf("FAIL unicast without a MAC accepted\n");
  if (udp_sender_template(&c, "10.1.2", 1, lmac, "10.1.2.4", 2, dmac)) fails++, std::printf("FAIL bad local address accepted\n");
  if (udp_sender_template(&c, "10.1.2.3", 1, lmac, "nowhere", 2, dmac)) fails++, std::printf("FAIL bad dest address accepted\n");

  std::printf(fails ? "FAILED (%d)\n" : "PASS\n", fails);
  return fails ? 1 : 0;
}
