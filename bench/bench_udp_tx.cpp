// pn_udp_build on device-resident messages into 2-KiB slots (frame_off 8, Efvi's pkt_buf layout), 1024 channels,
// payloads packed back to back (so every source alignment occurs), against two yardsticks in the same run.
//   a  1472-B payloads, PN_UB_EFVI
//   b  the same, PN_UB_CSUM (the RFC 768 checksum summed on the way)
//   c  64-B payloads, PN_UB_EFVI
//   d  64-B payloads, PN_UB_CSUM
//   e  copy only: hipMemcpy2DAsync device-to-device of the same messages x 1514 bytes into the same slots
//   f  checksum only: pn_tx_fill(PN_TX_UDP) over the ring (a) left
// One process, the legs interleaved step by step (a, f, b, c, d, e), HIP events around each, the median of `steps`
// after 5 warm-up steps; every leg's output is checked once (a sample of slots from both ends and the middle of the
// ring against frames built on the host).  One JSON line.
//   bench_udp_tx [steps = 30] [messages = 1048576]
// (built by `make bench/bench_udp_tx`)
#include <arpa/inet.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/pollnet_amd.h"

namespace {

constexpr uint32_t kStride = 2048, kOff = 8, kBig = 1472, kSmall = 64, kChans = 1024, kWarm = 5, kSample = 1024;

#define HIP(x)                                                     \
  do {                                                             \
    hipError_t e_ = (x);                                           \
    if (e_ != hipSuccess) {                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 5;                                                    \
    }                                                              \
  } while (0)
#define PN(x)                                                    \
  do {                                                           \
    if (x) {                                                     \
      std::fprintf(stderr, "%s: %s\n", #x, pn_last_error(ctx));  \
      return 6;                                                  \
    }                                                            \
  } while (0)

double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

uint32_t ones_sum(const uint8_t* p, size_t n, uint32_t s = 0) { // big-endian words, odd tail zero-padded
  for (size_t i = 0; i + 1 < n; i += 2) s += (uint32_t)p[i] << 8 | p[i + 1];
  if (n & 1) s += (uint32_t)p[n - 1] << 8;
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return s;
}

pn_udp_channel channel_of(uint32_t k) { // 32 groups x 32 ports, init_udp_pkt's fields (Efvi.h:597-644)
  pn_udp_channel c{};
  uint8_t* h = c.hdr;
  const uint32_t dst = htonl(0xEF010100u + (k >> 5)), src = htonl(0x0A140000u + k);
  const uint16_t dp = htons((uint16_t)(20000 + (k & 31))), sp = htons((uint16_t)(40000 + (k & 7)));
  h[0] = 1, h[2] = 0x5e, h[3] = 1, h[4] = 1, h[5] = (uint8_t)(k >> 5);
  h[6] = 0, h[7] = 0x0f, h[8] = 0x53, h[11] = 1;
  h[12] = 0x08, h[14] = 0x45, h[20] = 0x40, h[22] = 64, h[23] = 17;
  std::memcpy(h + 26, &src, 4);
  std::memcpy(h + 30, &dst, 4);
  std::memcpy(h + 34, &sp, 2);
  std::memcpy(h + 36, &dp, 2);
  h[39] = 8;
  return c;
}

uint32_t chan_of(uint32_t i) { return (i * 2654435761u >> 12) % kChans; }

// What a built frame must be, on the host: Efvi's arithmetic for the IPv4 checksum (Efvi.h:405-411, 615-619), or
// the standard fold plus the RFC 768 checksum.
void expect_frame(uint8_t* f, const pn_udp_channel& c, const uint8_t* pay, uint32_t len, bool csum) {
  std::memcpy(f, c.hdr, 42);
  std::memcpy(f + 42, pay, len);
  const uint16_t tot = htons(28 + len), ul = htons(8 + len);
  std::memcpy(f + 16, &tot, 2);
  std::memcpy(f + 38, &ul, 2);
  f[24] = f[25] = f[40] = f[41] = 0;
  if (!csum) {
    uint16_t w[10];
    std::memcpy(w, f + 14, 20);
    uint32_t cache = 0;
    for (int i = 0; i < 10; i++) cache += i == 1 ? 0 : w[i];
    cache = (cache >> 16) + (cache & 0xffff);
    cache += cache >> 16;
    uint32_t ipsum = cache + tot;
    ipsum += ipsum >> 16;
    const uint16_t chk = ~ipsum & 0xffff;
    std::memcpy(f + 24, &chk, 2);
    return;
  }
  uint32_t s = (~ones_sum(f + 14, 20)) & 0xffff;
  f[24] = s >> 8, f[25] = s & 0xff;
  uint8_t ph[12];
  std::memcpy(ph, f + 26, 8);
  ph[8] = 0, ph[9] = 17, ph[10] = f[38], ph[11] = f[39];
  s = (~ones_sum(f + 34, 8 + len, ones_sum(ph, 12))) & 0xffff;
  if (s == 0) s = 0xffff;
  f[40] = s >> 8, f[41] = s & 0xff;
}

} // namespace

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 30;
  const uint32_t n = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1u << 20;
  if (steps < 1 || n < 4 * kSample) {
    std::fprintf(stderr, "usage: bench_udp_tx [steps >= 1] [messages >= %u]\n", 4 * kSample);
    return 2;
  }
  pn_ctx* ctx = nullptr;
  if (pn_open(0, &ctx)) {
    std::fprintf(stderr, "pn_open: %s\n", pn_last_error(nullptr));
    return 3;
  }
  std::vector<pn_udp_channel> chans(kChans);
  for (uint32_t k = 0; k < kChans; k++) chans[k] = channel_of(k);
  PN(pn_udp_set_channels(ctx, chans.data(), kChans));

  // payloads: n x 1514 random bytes on the device (leg e copies whole 1514-B rows; the builds read the first
  // n x 1472 resp. n x 64 of them, message i at i * len: back to back), replicated from one host tile
  const size_t pay_bytes = (size_t)n * (kBig + 42);
  const size_t tile = 16u << 20;
  std::vector<uint8_t> host(tile);
  {
    std::mt19937 rng(1472);
    uint32_t* w = (uint32_t*)host.data();
    for (size_t i = 0; i < tile / 4; i++) w[i] = rng();
  }
  uint8_t *d_pay, *d_ring;
  HIP(hipMalloc((void**)&d_pay, pay_bytes + 16));
  for (size_t at = 0; at < pay_bytes; at += tile)
    HIP(hipMemcpy(d_pay + at, host.data(), std::min(tile, pay_bytes - at), hipMemcpyHostToDevice));
  auto pay_at = [&](size_t off) { return host.data() + off % tile; }; // tile boundaries are multiples of the tile
  HIP(hipMalloc((void**)&d_ring, (size_t)n * kStride));
  HIP(hipMemset(d_ring, 0, (size_t)n * kStride));

  std::vector<uint64_t> offs_big(n), offs_small(n);
  std::vector<uint16_t> lens_big(n, (uint16_t)kBig), lens_small(n, (uint16_t)kSmall);
  std::vector<uint32_t> chan_ids(n);
  for (uint32_t i = 0; i < n; i++) {
    offs_big[i] = (uint64_t)i * kBig;
    offs_small[i] = (uint64_t)i * kSmall;
    chan_ids[i] = chan_of(i);
  }
  uint64_t *d_offs_big, *d_offs_small;
  uint16_t *d_lens_big, *d_lens_small, *d_flens;
  uint32_t* d_chans;
  HIP(hipMalloc((void**)&d_offs_big, 8 * (size_t)n));
  HIP(hipMalloc((void**)&d_offs_small, 8 * (size_t)n));
  HIP(hipMalloc((void**)&d_lens_big, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_lens_small, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_flens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_chans, 4 * (size_t)n));
  HIP(hipMemcpy(d_offs_big, offs_big.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_offs_small, offs_small.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lens_big, lens_big.data(), 2 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lens_small, lens_small.data(), 2 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_chans, chan_ids.data(), 4 * (size_t)n, hipMemcpyHostToDevice));

  hipStream_t s;
  HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  HIP(hipEventCreate(&e0));
  HIP(hipEventCreate(&e1));

  // a sample of slots (both ends and the middle) of the ring as it is now, and of frame_lens
  const uint32_t sample_at[3] = {0, n / 2 - kSample / 2, n - kSample};
  std::vector<uint8_t> got((size_t)kSample * kStride), want(kStride);
  std::vector<uint16_t> flens(kSample);
  int bad = 0;
  auto check = [&](const char* leg, uint32_t len, int kind) -> int { // kind 0 efvi, 1 csum, 2 copy, 3 fill
    for (uint32_t base : sample_at) {
      HIP(hipMemcpy(got.data(), d_ring + (size_t)base * kStride, got.size(), hipMemcpyDeviceToHost));
      HIP(hipMemcpy(flens.data(), d_flens + base, 2 * kSample, hipMemcpyDeviceToHost));
      for (uint32_t r = 0; r < kSample; r++) {
        const uint32_t i = base + r;
        const uint8_t* f = got.data() + (size_t)r * kStride + kOff;
        bool ok;
        if (kind == 2) {
          ok = true;
          for (uint32_t b = 0; b < 1514 && ok; b++) ok = f[b] == *pay_at((size_t)i * 1514 + b);
        } else if (kind == 3) {
          ok = ones_sum(f + 14, 20) == 0xffff;
        } else {
          const size_t off = (size_t)i * len;
          std::vector<uint8_t> p(len);
          for (uint32_t b = 0; b < len; b++) p[b] = *pay_at(off + b);
          expect_frame(want.data(), chans[chan_of(i)], p.data(), len, kind == 1);
          ok = std::memcmp(f, want.data(), 42 + len) == 0 && flens[r] == 42 + len;
        }
        if (!ok && bad++ < 5) std::fprintf(stderr, "leg %s: slot %u is wrong\n", leg, i);
      }
    }
    return 0;
  };

  enum { A, F, B, C, D, E, kLegs };
  const char* names[kLegs] = {"a", "f", "b", "c", "d", "e"};
  std::vector<float> ms[kLegs];
  for (int step = 0; step < (int)kWarm + steps; step++) {
    for (int leg = 0; leg < kLegs; leg++) {
      HIP(hipEventRecord(e0, s));
      switch (leg) {
        case A: PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kBig, d_offs_big, d_lens_big, d_chans, d_ring, kStride, kOff, n, PN_UB_EFVI, d_flens, s)); break;
        case B: PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kBig, d_offs_big, d_lens_big, d_chans, d_ring, kStride, kOff, n, PN_UB_CSUM, d_flens, s)); break;
        case C: PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kSmall, d_offs_small, d_lens_small, d_chans, d_ring, kStride, kOff, n, PN_UB_EFVI, d_flens, s)); break;
        case D: PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kSmall, d_offs_small, d_lens_small, d_chans, d_ring, kStride, kOff, n, PN_UB_CSUM, d_flens, s)); break;
        case E: HIP(hipMemcpy2DAsync(d_ring + kOff, kStride, d_pay, 1514, 1514, n, hipMemcpyDeviceToDevice, s)); break;
        case F: PN(pn_tx_fill(ctx, d_ring, kStride, kOff, n, nullptr, PN_TX_UDP, s)); break;
      }
      HIP(hipEventRecord(e1, s));
      HIP(hipEventSynchronize(e1));
      float t;
      HIP(hipEventElapsedTime(&t, e0, e1));
      if (step >= (int)kWarm) ms[leg].push_back(t);
      if (step == 0) {
        const int rc = check(names[leg], leg == C || leg == D ? kSmall : kBig,
                             leg == E ? 2 : leg == F ? 3 : (leg == B || leg == D) ? 1 : 0);
        if (rc) return rc;
      }
    }
  }
  double med[kLegs];
  for (int leg = 0; leg < kLegs; leg++) med[leg] = median(ms[leg]);
  const double big_bytes = (double)n * (42 + kBig), small_bytes = (double)n * (42 + kSmall);
  auto gbs = [](double bytes, double msec) { return bytes / msec / 1e6; };
  std::printf(
      "{\"bench\": \"udp_tx\", \"messages\": %u, \"steps\": %d, \"slot_stride\": %u, \"frame_off\": %u, \"channels\": %u, "
      "\"a_1472_efvi_ms\": %.4f, \"b_1472_csum_ms\": %.4f, \"c_64_efvi_ms\": %.4f, \"d_64_csum_ms\": %.4f, "
      "\"e_memcpy2d_1514_ms\": %.4f, \"f_tx_fill_udp_ms\": %.4f, "
      "\"a_written_GBps\": %.1f, \"b_written_GBps\": %.1f, \"c_written_GBps\": %.1f, \"d_written_GBps\": %.1f, "
      "\"e_written_GBps\": %.1f, \"a_Mmsgs\": %.1f, \"c_Mmsgs\": %.1f, "
      "\"a_over_e\": %.3f, \"b_over_a\": %.3f, \"b_over_e_plus_f\": %.3f, \"d_over_c\": %.3f, \"outputs_ok\": %s}\n",
      n, steps, kStride, kOff, kChans, med[A], med[B], med[C], med[D], med[E], med[F], gbs(big_bytes, med[A]),
      gbs(big_bytes, med[B]), gbs(small_bytes, med[C]), gbs(small_bytes, med[D]), gbs(big_bytes, med[E]),
      n / med[A] / 1e3, n / med[C] / 1e3, med[A] / med[E], med[B] / med[A], med[B] / (med[E] + med[F]), med[D] / med[C],
      bad ? "false" : "true");
  pn_close(ctx);
  return bad ? 1 : 0;
}
