// pn_udp_demux on device-resident 2-KiB slots (frame_off 8) against pn_udp_gather on the same ring and records in the
// same run.  The rings are built once by pn_udp_build (PN_UB_CSUM) from random payloads and classified once.
//   a  1472-B datagrams, 1,024 subscriptions drawn uniformly
//   b  1472-B datagrams, 1 subscription
//   c  1472-B datagrams, 4,096 subscriptions drawn uniformly
//   d  64-B datagrams, 1,024 subscriptions
//   e  1472-B datagrams, one frame in 16 taken (the others are for destinations nobody subscribed to), 1,024
// Each leg twice: x_demux (pn_udp_demux, n_subs = the leg's subscriptions) and x_gather (pn_udp_gather, the yardstick).
// One process, the legs interleaved step by step, HIP events around each, the median of `steps` after 5 warm-up
// steps; every demux's output is checked once: the total against the gather's for the same ring, sub_first / sub_bytes
// at both ends, and a sample of messages from both ends and the middle (grouped, in arrival order within a
// subscription, offsets the running sum, the bytes those the ring was built from).  One JSON line.
//   bench_udp_demux [steps = 30] [slots = 1048576]
// (built by `make bench/bench_udp_demux`)
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

constexpr uint32_t kStride = 2048, kOff = 8, kBig = 1472, kSmall = 64, kWarm = 5, kSample = 1024, kRings = 5;

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

pn_udp_channel channel_of(uint32_t k) { // 128 groups x 32 ports
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

uint32_t draw(uint32_t i, uint32_t mod) { return (i * 2654435761u >> 12) % mod; }

struct Leg {
  const char* name;
  uint32_t len, n_subs, every;
};
const Leg kLeg[kRings] = {{"a", kBig, 1024, 1}, {"b", kBig, 1, 1}, {"c", kBig, 4096, 1}, {"d", kSmall, 1024, 1},
                          {"e", kBig, 1024, 16}};
// frame i's channel in ring r: a subscription's for a taken frame, one nobody subscribed to (ring e only) otherwise
uint32_t chan_of(int r, uint32_t i) {
  const Leg& l = kLeg[r];
  return i % l.every == 0 ? draw(i, l.n_subs) : 1024 + draw(i, 1024);
}

} // namespace

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 30;
  const uint32_t n = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1u << 20;
  if (steps < 1 || n < 64 * kSample || n % 16 || n > PN_UDP_DEMUX_MAX_N) {
    std::fprintf(stderr, "usage: bench_udp_demux [steps >= 1] [slots >= %u, a multiple of 16]\n", 64 * kSample);
    return 2;
  }
  pn_ctx* ctx = nullptr;
  if (pn_open(0, &ctx)) {
    std::fprintf(stderr, "pn_open: %s\n", pn_last_error(nullptr));
    return 3;
  }
  std::vector<pn_udp_channel> chans(PN_UDP_MAX_CHANNELS);
  std::vector<pn_udp_sub> subs(PN_UDP_MAX_SUBS);
  for (uint32_t k = 0; k < PN_UDP_MAX_CHANNELS; k++) chans[k] = channel_of(k);
  for (uint32_t k = 0; k < PN_UDP_MAX_SUBS; k++) {
    std::memcpy(&subs[k].dst_ip, chans[k].hdr + 30, 4);
    std::memcpy(&subs[k].dst_port, chans[k].hdr + 36, 2);
    subs[k]._pad = 0;
  }
  PN(pn_udp_set_channels(ctx, chans.data(), PN_UDP_MAX_CHANNELS));

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
  uint8_t *d_pay, *d_out, *d_ring[kRings];
  HIP(hipMalloc((void**)&d_pay, pay_bytes + 16));
  HIP(hipMalloc((void**)&d_out, pay_bytes));
  for (size_t at = 0; at < pay_bytes; at += tile)
    HIP(hipMemcpy(d_pay + at, host.data(), std::min(tile, pay_bytes - at), hipMemcpyHostToDevice));
  for (auto& r : d_ring) {
    HIP(hipMalloc((void**)&r, (size_t)n * kStride));
    HIP(hipMemset(r, 0xA5, (size_t)n * kStride)); // non-zero after every datagram
  }

  std::vector<uint64_t> offs(n);
  std::vector<uint16_t> lens(n);
  std::vector<uint32_t> chan_ids(n);
  uint64_t *d_offs, *g_offs, *g_sbytes;
  uint16_t *d_lens, *d_flens, *g_lens;
  uint32_t *d_chans, *g_subs, *g_src, *g_first;
  pn_udp_result* d_rec[kRings];
  pn_udp_gather_total* d_total;
  HIP(hipMalloc((void**)&d_offs, 8 * (size_t)n));
  HIP(hipMalloc((void**)&d_lens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_flens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&d_chans, 4 * (size_t)n));
  HIP(hipMalloc((void**)&g_offs, 8 * (size_t)n));
  HIP(hipMalloc((void**)&g_lens, 2 * (size_t)n));
  HIP(hipMalloc((void**)&g_subs, 4 * (size_t)n));
  HIP(hipMalloc((void**)&g_src, 4 * (size_t)n));
  HIP(hipMalloc((void**)&g_first, 4 * (PN_UDP_MAX_SUBS + 1)));
  HIP(hipMalloc((void**)&g_sbytes, 8 * (PN_UDP_MAX_SUBS + 1)));
  for (auto& r : d_rec) HIP(hipMalloc((void**)&r, sizeof(pn_udp_result) * (size_t)n));
  HIP(hipMalloc((void**)&d_total, sizeof(pn_udp_gather_total)));

  hipStream_t s;
  HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  HIP(hipEventCreate(&e0));
  HIP(hipEventCreate(&e1));

  // the five rings and their records: 1,024 subscriptions set for all but ring c (every channel subscribed)
  for (int r = 0; r < (int)kRings; r++) {
    for (uint32_t i = 0; i < n; i++) {
      offs[i] = (uint64_t)i * kLeg[r].len;
      lens[i] = (uint16_t)kLeg[r].len;
      chan_ids[i] = chan_of(r, i);
    }
    HIP(hipMemcpy(d_offs, offs.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_lens, lens.data(), 2 * (size_t)n, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_chans, chan_ids.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    PN(pn_sync(ctx));
    PN(pn_udp_set_subs(ctx, subs.data(), r == 2 ? PN_UDP_MAX_SUBS : 1024));
    PN(pn_udp_build(ctx, d_pay, (uint64_t)n * kLeg[r].len, d_offs, d_lens, d_chans, d_ring[r], kStride, kOff, n, PN_UB_CSUM,
                    d_flens, s));
    PN(pn_udp_classify(ctx, d_ring[r], kStride, kOff, n, d_rec[r], s));
    HIP(hipStreamSynchronize(s));
  }

  int bad = 0;
  auto fail = [&](const char* leg, const char* what, uint64_t v) {
    if (bad++ < 8) std::fprintf(stderr, "leg %s: %s (%llu)\n", leg, what, (unsigned long long)v);
  };
  pn_udp_gather_total gather_total[kRings] = {};
  std::vector<uint8_t> got;
  std::vector<uint64_t> h_offs(kSample), h_sbytes(PN_UDP_MAX_SUBS + 1);
  std::vector<uint16_t> h_lens(kSample);
  std::vector<uint32_t> h_subs(kSample), h_src(kSample), h_first(PN_UDP_MAX_SUBS + 1);
  auto check_demux = [&](int r) -> int {
    const Leg& l = kLeg[r];
    pn_udp_gather_total t;
    HIP(hipMemcpy(&t, d_total, sizeof(t), hipMemcpyDeviceToHost));
    const uint32_t msgs = n / l.every;
    if (t.n_msgs != msgs || t.n_fit != msgs || t.n_bytes != (uint64_t)msgs * l.len) {
      fail(l.name, "demux total", t.n_msgs);
      return 0;
    }
    HIP(hipMemcpy(h_first.data(), g_first, 4 * (l.n_subs + 1), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_sbytes.data(), g_sbytes, 8 * (l.n_subs + 1), hipMemcpyDeviceToHost));
    if (h_first[0] != 0 || h_first[l.n_subs] != msgs || h_sbytes[0] != 0 || h_sbytes[l.n_subs] != t.n_bytes)
      fail(l.name, "sub_first / sub_bytes ends", h_first[l.n_subs]);
    for (uint32_t q = 0; q < l.n_subs; q++)
      if (h_first[q] > h_first[q + 1] || h_sbytes[q] != (uint64_t)h_first[q] * l.len) fail(l.name, "sub_first / sub_bytes", q);
    got.resize((size_t)kSample * l.len);
    const uint32_t sample_at[3] = {0, msgs / 2 - kSample / 2, msgs - kSample};
    for (uint32_t base : sample_at) {
      HIP(hipMemcpy(got.data(), d_out + (size_t)base * l.len, got.size(), hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_offs.data(), g_offs + base, 8 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_lens.data(), g_lens + base, 2 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_subs.data(), g_subs + base, 4 * kSample, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_src.data(), g_src + base, 4 * kSample, hipMemcpyDeviceToHost));
      for (uint32_t k = 0; k < kSample; k++) {
        const uint32_t j = base + k, i = h_src[k];
        bool ok = i < n && i % l.every == 0 && h_offs[k] == (uint64_t)j * l.len && h_lens[k] == l.len &&
                  h_subs[k] == chan_of(r, i) && h_first[h_subs[k]] <= j && j < h_first[h_subs[k] + 1];
        if (ok && k && h_subs[k] == h_subs[k - 1]) ok = h_src[k - 1] < i; // arrival order within a subscription
        if (ok && k && h_subs[k] != h_subs[k - 1]) ok = h_subs[k - 1] < h_subs[k];
        for (uint32_t b = 0; b < l.len && ok; b++) ok = got[(size_t)k * l.len + b] == *pay_at((size_t)i * l.len + b);
        if (!ok) fail(l.name, "message is wrong", j);
      }
    }
    return 0;
  };

  std::vector<float> ms[2 * kRings];
  for (int step = 0; step < (int)kWarm + steps; step++) {
    for (int leg = 0; leg < 2 * (int)kRings; leg++) {
      const int r = leg / 2;
      const bool demux = leg % 2 == 0;
      HIP(hipEventRecord(e0, s));
      if (demux)
        PN(pn_udp_demux(ctx, d_ring[r], kStride, kOff, n, d_rec[r], kLeg[r].n_subs, d_out, pay_bytes, g_offs, g_lens, g_subs,
                        g_src, g_first, g_sbytes, d_total, s));
      else
        PN(pn_udp_gather(ctx, d_ring[r], kStride, kOff, n, d_rec[r], d_out, pay_bytes, g_offs, g_lens, g_subs, g_src, d_total, s));
      HIP(hipEventRecord(e1, s));
      HIP(hipEventSynchronize(e1));
      float t;
      HIP(hipEventElapsedTime(&t, e0, e1));
      if (step >= (int)kWarm) ms[leg].push_back(t);
      if (step == 0) {
        if (demux) {
          if (const int rc = check_demux(r)) return rc;
        } else {
          HIP(hipMemcpy(&gather_total[r], d_total, sizeof(pn_udp_gather_total), hipMemcpyDeviceToHost));
          const uint32_t msgs = n / kLeg[r].every;
          if (gather_total[r].n_msgs != msgs || gather_total[r].n_bytes != (uint64_t)msgs * kLeg[r].len)
            fail(kLeg[r].name, "gather total", gather_total[r].n_msgs);
        }
      }
    }
  }
  std::printf("{\"bench\": \"udp_demux\", \"slots\": %u, \"steps\": %d, \"slot_stride\": %u, \"frame_off\": %u", n, steps, kStride,
              kOff);
  for (int r = 0; r < (int)kRings; r++) {
    const double dm = median(ms[2 * r]), ga = median(ms[2 * r + 1]);
    std::printf(", \"%s_len\": %u, \"%s_subs\": %u, \"%s_taken_1_in\": %u, \"%s_demux_ms\": %.4f, \"%s_gather_ms\": %.4f, "
                "\"%s_demux_over_gather\": %.3f",
                kLeg[r].name, kLeg[r].len, kLeg[r].name, kLeg[r].n_subs, kLeg[r].name, kLeg[r].every, kLeg[r].name, dm,
                kLeg[r].name, ga, kLeg[r].name, dm / ga);
  }
  std::printf(", \"outputs_ok\": %s}\n", bad ? "false" : "true");
  pn_close(ctx);
  return bad ? 1 : 0;
}
