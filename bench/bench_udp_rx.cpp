// pn_udp_classify and pn_udp_classify_indexed on device-resident 2-KiB slots against pn_classify in the same run.
//   a  every frame a 1514-B UDP datagram for one of 1024 subscriptions, valid non-zero checksum, verified
//   b  the same frames sent with checksum 0 (Efvi's sender): one header line each
//   c  one frame in 16 subscribed, the rest to other ports: only our own traffic is streamed
//   d  pn_classify on C2 TCP frames of the same size (the generator's), the yardstick: (a) moves the same bytes
//   e  (a)'s ring through pn_udp_classify_indexed with offsets[i] = i * stride + frame_off: what the indexed entry
//      point costs over the strided one on the same bytes (e_over_a)
//   f  (c)'s ring the same way (f_over_c)
// One process, the six legs interleaved step by step, HIP events around each launch, the median of `steps` after
// warm-up; every leg's records are checked once, (e) and (f) to be (a)'s and (c)'s byte for byte.  One JSON line.
//   bench_udp_rx [steps = 30] [frames = 1048576]
// (built by `make bench/bench_udp_rx`)
#include <arpa/inet.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/pollnet_amd_gen.h"

namespace {

constexpr uint32_t kStride = 2048, kOff = 2, kPayload = 1472, kSubs = 1024, kTile = 1u << 14; // frames per host tile

#define HIP(x)                                                                        \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
      return 5;                                                                       \
    }                                                                                 \
  } while (0)

double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

uint32_t ones_sum(const uint8_t* p, size_t n, uint32_t s = 0) {
  for (size_t i = 0; i + 1 < n; i += 2) s += (uint32_t)p[i] << 8 | p[i + 1];
  if (n & 1) s += (uint32_t)p[n - 1] << 8;
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return s;
}

pn_udp_sub sub_of(uint32_t k) { // 32 groups x 32 ports
  pn_udp_sub s{};
  s.dst_ip = htonl(0xEF010100u + (k >> 5));
  s.dst_port = htons((uint16_t)(20000 + (k & 31)));
  return s;
}

// One 1514-B UDP frame for subscription k (port_shift != 0: the same group, a port nobody subscribed to).
void put_frame(uint8_t* slot, std::mt19937& rng, uint32_t k, uint32_t port_shift, bool zero_csum) {
  std::memset(slot, 0, kStride);
  uint8_t* eth = slot + kOff;
  eth[6] = 2, eth[11] = 1, eth[12] = 0x08;
  uint8_t* ip = eth + 14;
  const uint32_t tot = 28 + kPayload, ulen = 8 + kPayload;
  ip[0] = 0x45, ip[2] = tot >> 8, ip[3] = tot & 0xff, ip[6] = 0x40, ip[8] = 64, ip[9] = 17;
  const uint32_t src = htonl(0x0A000000u + (rng() & 0xffffff));
  const pn_udp_sub s = sub_of(k);
  const uint16_t dport = htons((uint16_t)(ntohs(s.dst_port) + port_shift)), sport = htons((uint16_t)(1024 + rng() % 60000));
  std::memcpy(ip + 12, &src, 4);
  std::memcpy(ip + 16, &s.dst_ip, 4);
  uint32_t c = (~ones_sum(ip, 20)) & 0xffff;
  ip[10] = c >> 8, ip[11] = c & 0xff;
  uint8_t* udp = ip + 20;
  std::memcpy(udp, &sport, 2);
  std::memcpy(udp + 2, &dport, 2);
  udp[4] = ulen >> 8, udp[5] = ulen & 0xff;
  uint32_t* w = (uint32_t*)(udp + 8); // udp + 8 = slot + 44: 4-byte aligned
  for (uint32_t i = 0; i < kPayload / 4; i++) w[i] = rng();
  if (!zero_csum) {
    uint8_t ph[12];
    std::memcpy(ph, ip + 12, 8);
    ph[8] = 0, ph[9] = 17, ph[10] = udp[4], ph[11] = udp[5];
    c = (~ones_sum(udp, ulen, ones_sum(ph, 12))) & 0xffff;
    if (c == 0) c = 0xffff;
    udp[6] = c >> 8, udp[7] = c & 0xff;
  }
}

} // namespace

int main(int argc, char** argv) {
  const uint32_t steps = argc > 1 ? std::max(20, std::atoi(argv[1])) : 30;
  const uint32_t n = argc > 2 ? (uint32_t)std::atoi(argv[2]) : (1u << 20);
  const uint32_t warmup = 5;
  if (n == 0 || n % 16) return std::fprintf(stderr, "frames must be a positive multiple of 16\n"), 2;
  const size_t ring_bytes = (size_t)n * kStride;

  pn_ctx* ctx = nullptr;
  if (pn_open(0, &ctx)) return std::fprintf(stderr, "%s\n", pn_last_error(nullptr)), 4;
  hipStream_t s;
  HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  constexpr int kLegs = 6;
  uint8_t* ring[4] = {};
  void* rec[kLegs] = {};
  for (int l = 0; l < 4; l++) HIP(hipMalloc((void**)&ring[l], ring_bytes));
  for (int l = 0; l < kLegs; l++) HIP(hipMalloc(&rec[l], (size_t)n * 16));
  uint64_t* offs = nullptr; // legs e, f: every slot's Ethernet header, in slot order
  HIP(hipMalloc((void**)&offs, (size_t)n * sizeof(uint64_t)));
  {
    std::vector<uint64_t> host(n);
    for (uint32_t i = 0; i < n; i++) host[i] = (uint64_t)i * kStride + kOff;
    HIP(hipMemcpy(offs, host.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  }

  // legs a, b, c: host tiles of kTile distinct frames, repeated along the ring (every slot has its own address:
  // nothing is served from a cache twice within a launch)
  {
    const uint32_t tile = std::min(kTile, n);
    std::vector<uint8_t> host((size_t)tile * kStride);
    for (int l = 0; l < 3; l++) {
      std::mt19937 rng(1234 + l);
      for (uint32_t i = 0; i < tile; i++) {
        const bool ours = l != 2 || i % 16 == 5;
        put_frame(host.data() + (size_t)i * kStride, rng, rng() % kSubs, ours ? 0 : 32 + rng() % 1000, l == 1);
      }
      for (uint32_t base = 0; base < n; base += tile)
        HIP(hipMemcpy(ring[l] + (size_t)base * kStride, host.data(), (size_t)std::min(tile, n - base) * kStride,
                      hipMemcpyHostToDevice));
    }
  }
  // leg d: the generator's C2 frames and table
  {
    pn_gen_params gp{2, 1, 0, 1024, 0x5EED0002};
    std::vector<uint8_t> host(ring_bytes);
    if (pn_gen_frames(&gp, 0, n, host.data(), kStride, kOff, 16)) return 3;
    HIP(hipMemcpy(ring[3], host.data(), ring_bytes, hipMemcpyHostToDevice));
    pn_conn_table* t = nullptr;
    if (pn_table_create(1024, 1024, &t) || pn_gen_conn_table(&gp, t)) return 3;
    uint32_t ne = 0;
    uint64_t mask = 0;
    const pn_conn_entry* e = pn_table_entries(t, &ne, &mask);
    if (pn_set_conn_table(ctx, e, ne, mask, 1024)) return std::fprintf(stderr, "%s\n", pn_last_error(ctx)), 4;
    pn_table_destroy(t);
  }
  {
    std::vector<pn_udp_sub> subs(kSubs);
    for (uint32_t k = 0; k < kSubs; k++) subs[k] = sub_of(k);
    if (pn_udp_set_subs(ctx, subs.data(), kSubs)) return std::fprintf(stderr, "%s\n", pn_last_error(ctx)), 4;
  }

  auto launch = [&](int l) {
    if (l < 3) return pn_udp_classify(ctx, ring[l], kStride, kOff, n, rec[l], s);
    if (l == 3) return pn_classify(ctx, ring[3], kStride, kOff, n, rec[3], s);
    return pn_udp_classify_indexed(ctx, ring[l == 4 ? 0 : 2], offs, kOff % 16, n, kStride - kOff, rec[l], s);
  };
  hipEvent_t ev0, ev1;
  HIP(hipEventCreate(&ev0));
  HIP(hipEventCreate(&ev1));
  std::vector<float> ms[kLegs];
  for (uint32_t step = 0; step < warmup + steps; step++) {
    for (int l = 0; l < kLegs; l++) {
      HIP(hipEventRecord(ev0, s));
      if (launch(l)) return std::fprintf(stderr, "%s\n", pn_last_error(ctx)), 4;
      HIP(hipEventRecord(ev1, s));
      HIP(hipEventSynchronize(ev1));
      float t = 0;
      HIP(hipEventElapsedTime(&t, ev0, ev1));
      if (step >= warmup) ms[l].push_back(t);
    }
  }

  // what each leg must have produced
  bool ok = true;
  uint64_t delivered[3] = {}, udp_ok[3] = {}, nocsum[3] = {}, tcp_ok = 0;
  {
    std::vector<pn_udp_result> r(n);
    for (int l = 0; l < 3; l++) {
      HIP(hipMemcpy(r.data(), rec[l], (size_t)n * 16, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; i++) {
        delivered[l] += PN_UDP_DELIVER(r[i].flags) ? 1 : 0;
        udp_ok[l] += (r[i].flags & PN_UF_UDP_OK) ? 1 : 0;
        nocsum[l] += (r[i].flags & PN_UF_NOCSUM) ? 1 : 0;
        ok = ok && (r[i].flags & PN_UF_IP_OK) && r[i].payload_len == kPayload;
      }
    }
    // the indexed legs wrote the strided legs' records
    std::vector<pn_udp_result> r2(n);
    for (int l = 4; l < kLegs; l++) {
      HIP(hipMemcpy(r.data(), rec[l == 4 ? 0 : 2], (size_t)n * 16, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(r2.data(), rec[l], (size_t)n * 16, hipMemcpyDeviceToHost));
      ok = ok && std::memcmp(r.data(), r2.data(), (size_t)n * 16) == 0;
    }
    std::vector<pn_result> q(n);
    HIP(hipMemcpy(q.data(), rec[3], (size_t)n * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) tcp_ok += (q[i].flags & PN_F_TCP_OK) ? 1 : 0;
  }
  ok = ok && delivered[0] == n && udp_ok[0] == n && delivered[1] == n && nocsum[1] == n && delivered[2] == n / 16 &&
       udp_ok[2] == n / 16 && tcp_ok + (n + 1023) / 1024 >= n; // the generator damages one C2 frame in 1024

  const double a = median(ms[0]), b = median(ms[1]), c = median(ms[2]), d = median(ms[3]);
  const double e_ms = median(ms[4]), f_ms = median(ms[5]);
  const double wire_bits = 8.0 * 1514 * n;
  std::printf(
      "{\"bench\": \"udp_rx\", \"frames\": %u, \"slot_stride\": %u, \"frame_bytes\": 1514, \"subscriptions\": %u, \"steps\": %u, "
      "\"warmup\": %u, \"a_verified_ms\": %.4f, \"b_checksum0_ms\": %.4f, \"c_one_in_16_ms\": %.4f, \"d_tcp_classify_ms\": %.4f, "
      "\"a_over_d\": %.4f, \"b_over_d\": %.4f, \"c_over_d\": %.4f, \"a_gbit_s\": %.1f, \"d_gbit_s\": %.1f, "
      "\"a_min_ms\": %.4f, \"d_min_ms\": %.4f, \"e_indexed_verified_ms\": %.4f, \"f_indexed_one_in_16_ms\": %.4f, "
      "\"e_over_a\": %.4f, \"f_over_c\": %.4f, \"e_min_ms\": %.4f, \"f_min_ms\": %.4f, \"ok\": %s}\n",
      n, kStride, kSubs, steps, warmup, a, b, c, d, a / d, b / d, c / d, wire_bits / (a * 1e6), wire_bits / (d * 1e6),
      (double)*std::min_element(ms[0].begin(), ms[0].end()), (double)*std::min_element(ms[3].begin(), ms[3].end()),
      e_ms, f_ms, e_ms / a, f_ms / c, (double)*std::min_element(ms[4].begin(), ms[4].end()),
      (double)*std::min_element(ms[5].begin(), ms[5].end()), ok ? "true" : "false");
  (void)hipStreamSynchronize(s);
  for (int l = 0; l < 4; l++) (void)hipFree(ring[l]);
  for (int l = 0; l < kLegs; l++) (void)hipFree(rec[l]);
  (void)hipFree(offs);
  pn_close(ctx);
  return ok ? 0 : 1;
}
