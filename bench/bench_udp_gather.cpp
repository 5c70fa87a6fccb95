// pn_udp_gather on device-resident 2-KiB slots (frame_off 8), 1,024 subscriptions, against three yardsticks in the
// same run.  The rings are built once by pn_udp_build (PN_UB_CSUM) from random payloads and classified once.
//   a  gather alone, 1472-B datagrams, every frame taken
//   b  pn_udp_classify (verifying) + gather on the same ring, one after the other on the stream
//   c  gather alone, 64-B datagrams, every frame taken
//   d  gather alone, 1472-B datagrams, one frame in 16 taken (the others are for destinations nobody subscribed to)
//   y  pn_udp_classify alone on the ring of (a)
//   p  pn_udp_build (PN_UB_PLAIN) of the same messages into a ring of the same kind: the inverse of (a)
//   q  the same build in PN_UB_CSUM
//   m  hipMemcpyAsync device-to-device of the bytes (a) writes
// One process, the legs interleaved step by step, HIP events around each, the median of `steps` after 5 warm-up
// steps; every gather's output is checked once (the total, and a sample of messages from both ends and the middle
// against the payloads the rings were built from).  One JSON line.
//   bench_udp_gather [steps = 30] [slots = 1048576]
// (built by `make bench/bench_udp_gather`)
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

constexpr uint32_t kStride = 2048, kOff = 8, kBig = 1472, kSmall = 64, kSubs = 1024, kWarm = 5, kSample = 1024;

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

pn_udp_channel channel_of(uint32_t k) { // 64 groups x 32 ports; the first 1,024 are subscribed to
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

uint32_t chan_of(uint32_t i) { return (i * 2654435761u >> 12) % kSubs; }

} // namespace

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 30;
  const uint32_t n = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1u << 20;
  if (steps < 1 || n < 64 * kSample || n % 16) {
    std::fprintf(stderr, "usage: bench_udp_gather [steps >= 1] [slots >= %u, a multiple of 16]\n", 64 * kSample);
    return 2;
  }
  pn_ctx* ctx = nullptr;
  if (pn_open(0, &ctx)) {
    std::fprintf(stderr, "pn_open: %s\n", pn_last_error(nullptr));
    return 3;
  }
  std::vector<pn_udp_channel> chans(2 * kSubs);
  std::vector<pn_udp_sub> subs(kSubs);
  for (uint32_t k = 0; k < 2 * kSubs; k++) chans[k] = channel_of(k);
  for (uint32_t k = 0; k < kSubs; k++) {
    std::memcpy(&subs[k].dst_ip, chans[k].hdr + 30, 4);
    std::memcpy(&subs[k].dst_port, chans[k].hdr + 36, 2);
    subs[k]._pad = 0;
  }
  PN(pn_udp_set_channels(ctx, chans.data(), 2 * kSubs));
  PN(pn_udp_set_subs(ctx, subs.data(), kSubs));

  // payloads: n x 1472 random bytes on the device, replicated from one host tile; message i at i * len
  const size_t pay_bytes = (size_t)n * kBig;
  const size_t tile = 16u << 20;
  std::vector<uint8_t> host(tile);
  {
    std::mt19937 rng(1472);
    uint32_t* w = (uint32_t*)host.data();
    for (size_t i = 0; i < tile / 4; i++) w[i] = rng();
  }
  auto pay_at = [&](size_t off) { return host.data() + off % tile; };
  uint8_t *d_pay, *d_out, *d_ring[4]; // rings: 1472-B all taken, 64-B, 1472-B 1 in 16 taken, the build yardstick's
  HIP(hipMalloc((void**)&d_pay, pay_bytes + 16));
  HIP(hipMalloc((void**)&d_out, pay_bytes));
  for (size_t at = 0; at < pay_bytes; at += tile)
    HIP(hipMemcpy(d_pay + at, host.data(), std::min(tile, pay_bytes - at), hipMemcpyHostToDevice));
  for (auto& r : d_ring) {
    HIP(hipMalloc((void**)&r, (size_t)n * kStride));
    HIP(hipMemset(r, 0xA5, (size_t)n * kStride)); // non-zero after every datagram
  }

  std::vector<uint64_t> offs_big(n), offs_small(n);
  std::vector<uint16_t> lens_big(n, (uint16_t)kBig), lens_small(n, (uint16_t)kSmall);
  std::vector<uint32_t> chan_ids(n), chan_sparse(n);
  for (uint32_t i = 0; i < n; i++) {
    offs_big[i] = (uint64_t)i * kBig;
    offs_small[i] = (uint64_t)i * kSmall;
    chan_ids[i] = chan_of(i);
    chan_sparse[i] = i % 16 == 0 ? chan_of(i) : kSubs + chan_of(i);
  }
  uint64_t *d_offs_big, *d_offs_small, *g_offs;
  uint16_t *d_lens_big, *d_lens_small, *d_flens, *g_lens;
  uint32_t *d_chans, *d_chans_sparse, *g_subs, *g_src;
  pn_udp_result* d_rec[4];
  pn_udp_gather_total* d_total;
  HIP(hipMalloc((void**)&d_offs_big, 8 * (size_t)n));
  HIP(hipMalloc((void**)&d_offs_small, 8 * (size_t)n));
  HIP(hipMalloc((void**)&d_lens_big, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_lens_small, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_flens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_chans, 4 * (size_t)n));
  HIP(hipMalloc((void**)&d_chans_sparse, 4 * (size_t)n));
  HIP(hipMalloc((void**)&g_offs, 8 * (size_t)n));
  HIP(hipMalloc((void**)&g_lens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&g_subs, 4 * (size_t)n));
  HIP(hipMalloc((void**)&g_src, 4 * (size_t)n));
  for (auto& r : d_rec) HIP(hipMalloc((void**)&r, sizeof(pn_udp_result) * (size_t)n));
  HIP(hipMalloc((void**)&d_total, sizeof(pn_udp_gather_total)));
  HIP(hipMemcpy(d_offs_big, offs_big.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_offs_small, offs_small.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lens_big, lens_big.data(), 2 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_lens_small, lens_small.data(), 2 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_chans, chan_ids.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_chans_sparse, chan_sparse.data(), 4 * (size_t)n, hipMemcpyHostToDevice));

  hipStream_t s;
  HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  HIP(hipEventCreate(&e0));
  HIP(hipEventCreate(&e1));

  // the three rings and their records
  PN(pn_udp_build(ctx, d_pay, pay_bytes, d_offs_big, d_lens_big, d_chans, d_ring[0], kStride, kOff, n, PN_UB_CSUM, d_flens, s));
  PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kSmall, d_offs_small, d_lens_small, d_chans, d_ring[1], kStride, kOff, n, PN_UB_CSUM, d_flens, s));
  PN(pn_udp_build(ctx, d_pay, pay_bytes, d_offs_big, d_lens_big, d_chans_sparse, d_ring[2], kStride, kOff, n, PN_UB_CSUM, d_flens, s));
  for (int r = 0; r < 3; r++) PN(pn_udp_classify(ctx, d_ring[r], kStride, kOff, n, d_rec[r], s));
  HIP(hipStreamSynchronize(s));

  // one gather's output: the total, and a sample of messages (both ends and the middle) against the payloads
  int bad = 0;
  std::vector<uint8_t> got;
  std::vector<uint64_t> h_offs(kSample);
  std::vector<uint16_t> h_lens(kSample);
  std::vector<uint32_t> h_subs(kSample), h_src(kSample);
  auto check = [&](const char* leg, uint32_t len, uint32_t every) -> int {
    pn_udp_gather_total t;
    HIP(hipMemcpy(&t, d_total, sizeof(t), hipMemcpyDeviceToHost));
    const uint32_t msgs = n / every;
    if (t.n_msgs != msgs || t.n_fit != msgs || t.n_bytes != (uint64_t)msgs * len) {
      if (bad++ < 5) std::fprintf(stderr, "leg %s: total {%llu, %u, %u}\n", leg, (unsigned long long)t.n_bytes, t.n_msgs, t.n_fit);
      return 0;
    }
    got.resize((size_t)kSample * len);
    const uint32_t sample_at[3] = {0, msgs / 2 - kSample / 2, msgs - kSample};
    for (uint32_t base : sample_at) {
      HIP(hipMemcpy(got.data(), d_out + (size_t)base * len, got.size(), hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_offs.data(), g_offs + base, 8 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_lens.data(), g_lens + base, 2 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_subs.data(), g_subs + base, 4 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_src.data(), g_src + base, 4 * kSample, hipMemcpyDeviceToHost));
      for (uint32_t r = 0; r < kSample; r++) {
        const uint32_t j = base + r, i = j * every;
        bool ok = h_offs[r] == (uint64_t)j * len && h_lens[r] == len && h_subs[r] == chan_of(i) && h_src[r] == i;
        for (uint32_t b = 0; b < len && ok; b++) ok = got[(size_t)r * len + b] == *pay_at((size_t)i * len + b);
        if (!ok && bad++ < 5) std::fprintf(stderr, "leg %s: message %u is wrong\n", leg, j);
      }
    }
    return 0;
  };
  auto gather = [&](int ring, pn_udp_result* rec) {
    return pn_udp_gather(ctx, d_ring[ring], kStride, kOff, n, rec, d_out, pay_bytes, g_offs, g_lens, g_subs, g_src, d_total, s);
  };

  enum { A, Y, B, P, C, Q, D, M, kLegs };
  std::vector<float> ms[kLegs];
  for (int step = 0; step < (int)kWarm + steps; step++) {
    for (int leg = 0; leg < kLegs; leg++) {
      HIP(hipEventRecord(e0, s));
      switch (leg) {
        case A: PN(gather(0, d_rec[0])); break;
        case B:
          PN(pn_udp_classify(ctx, d_ring[0], kStride, kOff, n, d_rec[3], s));
          PN(gather(0, d_rec[3]));
          break;
        case C: PN(gather(1, d_rec[1])); break;
        case D: PN(gather(2, d_rec[2])); break;
        case Y: PN(pn_udp_classify(ctx, d_ring[0], kStride, kOff, n, d_rec[3], s)); break;
        case P: PN(pn_udp_build(ctx, d_pay, pay_bytes, d_offs_big, d_lens_big, d_chans, d_ring[3], kStride, kOff, n, PN_UB_PLAIN, d_flens, s)); break;
        case Q: PN(pn_udp_build(ctx, d_pay, pay_bytes, d_offs_big, d_lens_big, d_chans, d_ring[3], kStride, kOff, n, PN_UB_CSUM, d_flens, s)); break;
        case M: HIP(hipMemcpyAsync(d_out, d_pay, pay_bytes, hipMemcpyDeviceToDevice, s)); break;
      }
      HIP(hipEventRecord(e1, s));
      HIP(hipEventSynchronize(e1));
      float t;
      HIP(hipEventElapsedTime(&t, e0, e1));
      if (step >= (int)kWarm) ms[leg].push_back(t);
      if (step == 0 && (leg == A || leg == B || leg == C || leg == D)) {
        const int rc = check(leg == A ? "a" : leg == B ? "b" : leg == C ? "c" : "d", leg == C ? kSmall : kBig, leg == D ? 16 : 1);
        if (rc) return rc;
      }
    }
  }
  double med[kLegs];
  for (int leg = 0; leg < kLegs; leg++) med[leg] = median(ms[leg]);
  auto gbs = [](double bytes, double msec) { return bytes / msec / 1e6; };
  std::printf(
      "{\"bench\": \"udp_gather\", \"slots\": %u, \"steps\": %d, \"slot_stride\": %u, \"frame_off\": %u, \"subscriptions\": %u, "
      "\"a_gather_1472_ms\": %.4f, \"b_classify_gather_1472_ms\": %.4f, \"c_gather_64_ms\": %.4f, "
      "\"d_gather_1_in_16_ms\": %.4f, \"y_classify_ms\": %.4f, \"p_build_plain_1472_ms\": %.4f, "
      "\"q_build_csum_1472_ms\": %.4f, \"m_memcpy_d2d_ms\": %.4f, "
      "\"a_payload_GBps\": %.1f, \"c_payload_GBps\": %.1f, \"m_GBps\": %.1f, \"a_Mmsgs\": %.1f, \"c_Mmsgs\": %.1f, "
      "\"a_over_p\": %.3f, \"a_over_q\": %.3f, \"a_over_m\": %.3f, \"b_over_y_plus_a\": %.3f, \"b_over_y\": %.3f, "
      "\"c_over_a\": %.3f, \"d_over_a\": %.3f, \"outputs_ok\": %s}\n",
      n, steps, kStride, kOff, kSubs, med[A], med[B], med[C], med[D], med[Y], med[P], med[Q], med[M],
      gbs((double)n * kBig, med[A]), gbs((double)n * kSmall, med[C]), gbs((double)n * kBig, med[M]), n / med[A] / 1e3,
      n / med[C] / 1e3, med[A] / med[P], med[A] / med[Q], med[A] / med[M], med[B] / (med[Y] + med[A]), med[B] / med[Y],
      med[C] / med[A], med[D] / med[A], bad ? "false" : "true");
  pn_close(ctx);
  return bad ? 1 : 0;
}
