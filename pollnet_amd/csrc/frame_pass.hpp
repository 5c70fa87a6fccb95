// The wave-per-64-frames frame pass shared by the RX classify kernel (rx_classify.hpp), the UDP receive kernels
// (udp_classify.hpp, udp_indexed.hpp) and the TX checksum fill (tx_fill.hpp): the 112-B header window of each
// frame (cooperative LDS tile or per-lane loads; load_window_strided for slots, load_window_indexed for frames
// named by offsets) and the wave-wide stream of every frame's summed extent past the window, with exact u16-word
// sums (v_dot2_u32_u16) transpose-reduced onto the frame's own lane.  Design and measurements: DESIGN.md §4.
#pragma once

#include <type_traits>

#include "device_common.hpp"

namespace pn_dev {

constexpr int kWave = 64;
constexpr int kFramesPerWave = 64; // one wave per 64-thread workgroup: +3 % over 4 waves/WG (profiles/r01_experiments)
constexpr int kBatch = 8;        // frames per stream batch: 16 x 1-KiB loads in flight per wave
// Cache policy (buffer-instruction aux bits on gfx950: 1 sc0, 2 nt, 16 sc1).  Frame
// bytes are read once: non-temporal loads.  Records are written once: write-through
// (sc1) stores.  Together -1.1..1.3 % kernel time (profiles/r01_experiments).
constexpr int kLoadAux = 2;
constexpr int kStoreAux = 16;

// Header window: kWinChunks x 16 B from the 16-B aligned chunk holding the IP
// header.  112 B ends on the slot's first 128-B line for the default layout (ip at
// slot+16), so the wave-wide stream starts on a fresh line.
constexpr int kWinChunks = 7;
constexpr int kWinBytes = 16 * kWinChunks;
using Window = Win<4 * kWinChunks>;

constexpr uint32_t kPadUnknown = 0xFFFFFFFFu;

// Flags of the frame pass (the ABL parameter of the RX kernel, SABL of the TX fill).  Each keeps the value it
// was measured under: the kernels' demangled names, which carry them, are keys in profiles/pmc_traffic.json.
// Timing-only ablations (records are wrong when set), for the same-run ceilings bench.py reports:
// bit0 skip the conn-table probe, bit1 skip the lane reduction.
enum : int { kAblNoProbe = 1, kAblNoReduce = 2 };
// Not an ablation: kExactRange bounds each frame's stream descriptor at its extent rounded
// up to a dword, so the hardware's per-dword range check zeroes the bytes past the extent
// and the per-dword tail masks go; a 2-mod-4 extent leaves 2 bytes of the last dword,
// subtracted on the lane that loaded them.
enum : int { kExactRange = 64 };
// kCoopProbe: conn-table lookups that continue past the home slot are finished by the whole
// wave, 64 entries per round trip (probe_finish in rx_classify.hpp).
enum : int { kCoopProbe = 256 };
// Not an ablation: a stream load whose whole 1-KiB range lies past the frame's extent (it would
// return zeros and fetch nothing) is not issued at all -- a wave-uniform branch on the frame's
// extent.  Mixed-size frames (most end inside the first KiB) skip up to half their load
// instructions; records are identical (the skipped loads' values were zero).
enum : int { kSkipEmptyLoads = 1024 };
// With kSkipEmptyLoads: the skipping form of phase 2 only in waves that have a frame ending inside
// its first stream KiB (one ballot per wave); a wave of full-size frames (every C2 wave) streams
// with unconditional loads, the form without the branches.
enum : int { kSkipWaveGate = 16384 };
// With kCoopProbe: the wave walks each distinct run position once for every lane standing at it
// (in C5's adversarial cluster, every cluster lane of a wave shares one home slot): one 64-entry
// round trip resolves all of them, each against its own key, instead of one round trip per lane.
// C5 -3.9 % (0.1660 -> 0.1596 ms; the probe's share over the no-probe ablation 13.6 -> 7.2 us),
// C3 equal (profiles/r03/probe_group_c{3,5}.json).
enum : int { kGroupProbe = 32768 };
// kSerialWindow: the window loads as they were until round 3, a branch around each (the compiler waits for
// each before issuing the next).  The RX kernel issues all 8 at once (C3 -3.8 %, C5 -4.3 %, C2 equal); the TX
// fill keeps the serial form, measured faster there (tx_fill.hpp, kTxStream).
enum : int { kSerialWindow = 1 << 20 };
// With kSkipWaveGate: phase 2 of full-size waves software-pipelined by half batches
// (stream_phase_pipelined; slot strides up to 2048).  C2 -1.4 %, C3/C5 unchanged (their waves take
// the skipping form), records identical (profiles/r03/pipe_stream/).  Pipelining the skipping form
// as well gained 0.2-0.7 % (not adopted); issuing every load so that all waves pipeline cost C3/C5 8 %.
enum : int { kPipeStream = 1 << 21 };
// Retired probe forms (measured, not adopted; DESIGN §4, profiles/r03/probe_ablation/): 2048 home slot + 3
// ahead, 65536 probe pipelined into phase 2, 262144 home entries through the scalar cache (code: commit 229bb94);
// 524288 a run-length hint in the device table's pad word sending long runs straight to the group walk (c3575ae).
// The other values that are no flag here (4 .. 32, 512, 4096, 8192, 131072, 1 << 22, 1 << 23) were A/B variants of
// the RX kernel, retired with their results in DESIGN §4, "Retired RX variants".
// product (pn_set_verify(ctx, 0)): no segment stream and no TCP verdict -- the header lines only, as the
// reference's release path reads them (Core::checksum is debug-only, Core.h:448-478)
enum : int { kHeaderOnly = 1 << 24 };
// product (the resident service, round 6): besides its record, each frame's chain fields go to KArgs::aux (device
// scratch, when set) -- the record again and the ack number, destination address, window and destination port --
// for the post's chain pass (rx_service.hip chain_pass)
enum : int { kChainAux = 1 << 25 };
// The production RX configuration.
constexpr int kProdAbl = kExactRange | kCoopProbe | kGroupProbe | kSkipEmptyLoads | kSkipWaveGate | kPipeStream;

// Header window of lane `lane`'s slot for a strided layout (slot r of the wave at
// r*stride from the descriptor base `rs`, window at slot + ipa_off).  Returns the
// slot's ether_type as stored (0x0008 = IPv4).
// COOP = 1: 8 lanes per slot load its 128-B window block -- the 16-B chunk before the
// window (ether_type) and the window -- into an XOR-swizzled LDS tile that each lane
// reads back.  When the window sits at line + 16 (the default frame_off = 2 layout) the
// block is the slot's first line: exactly one request per line.  Elsewhere it straddles
// two lines, still 8 slots per instruction instead of one window per lane.
// COOP = 0: each lane loads its own window (frame_off = 0, where no chunk precedes it).
// The cooperative window's LDS tile: 64 slots x 128 B (8 KiB), chunk p of slot r at
// r*8 + (p ^ (r&7)).  One static allocation per kernel.
__device__ __host__ __forceinline__ constexpr uint32_t coop_block(uint32_t ipa_off) { return ipa_off - 16; }
__device__ __forceinline__ u32x4* coop_tile() {
  __shared__ u32x4 tile[kFramesPerWave * 8];
  return tile;
}

// Whether 16-B part `part` of a window block starting at an address with low bits
// `blk_lo` is loaded.  When the header fields (ip .. ip+64) end in the block's first line,
// the parts in its second line are left out (zero in the tile): the stream starts at that
// line (stream_start) and would request it a second time.
template <int MIS>
__device__ __forceinline__ bool block_part_needed(uint32_t blk_lo, uint32_t part) {
  const uint32_t lo = blk_lo & 112u, s0 = 112u - lo;
  return MIS + 64 > (int)s0 || 16 * part < 128 - lo;
}

template <int MIS, int COOP, int LAUX, bool SERIAL = false>
__device__ __forceinline__ uint32_t load_window_strided(__amdgpu_buffer_rsrc_t rs, int lane, uint32_t stride,
                                                        uint32_t ipa_off, uint32_t base_lo, Window& h) {
  uint32_t ether_type;
  if constexpr (COOP) {
    static_assert(MIS + 64 <= kWinBytes, "window must cover ip .. ip+64");
    u32x4* tile = coop_tile();
    const uint32_t blk = coop_block(ipa_off);
    wave_lds_sync(); // a previous window's tile reads (a grouped kernel's last group) before these writes
    // All 8 loads in flight before the first LDS write: a part that is not needed gets an offset past
    // the descriptor's range (returns zeros, fetches nothing) instead of a branch around its load --
    // with the branches the compiler waited for each load before issuing the next (8 round trips).
    if constexpr (SERIAL) { // kSerialWindow (the TX fill): the round-1..3 form, a branch around each load
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (block_part_needed<MIS>(base_lo + r * stride + blk, part))
          v = __builtin_amdgcn_raw_buffer_load_b128(rs, r * stride + blk + 16 * part, 0, LAUX);
        tile[r * 8 + (part ^ (r & 7))] = v;
      }
    }
    u32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8 && !SERIAL; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      const uint32_t off = r * stride + blk + 16 * part;
      v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, block_part_needed<MIS>(base_lo + r * stride + blk, part) ? off : kNoFetch,
                                                   0, LAUX);
    }
#pragma unroll
    for (int i = 0; i < 8 && !SERIAL; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      tile[r * 8 + (part ^ (r & 7))] = v[i];
    }
    wave_lds_sync(); // each lane reads the rows other lanes wrote (the tile is this wave's own)
    constexpr uint32_t p0 = 1; // the window starts at the block's second chunk
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const u32x4 v = tile[lane * 8 + ((p0 + c) ^ (lane & 7))];
      h.d[4 * c + 0] = v.x;
      h.d[4 * c + 1] = v.y;
      h.d[4 * c + 2] = v.z;
      h.d[4 * c + 3] = v.w;
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = tile[lane * 8 + ((p0 - 1) ^ (lane & 7))].w >> 16;
  } else {
    const uint32_t lo = (uint32_t)lane * stride + ipa_off;
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, lo + 16 * c, 0, LAUX);
      h.d[4 * c + 0] = v.x;
      h.d[4 * c + 1] = v.y;
      h.d[4 * c + 2] = v.z;
      h.d[4 * c + 3] = v.w;
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = __builtin_amdgcn_raw_buffer_load_b32(rs, lo - 4, 0, LAUX) >> 16; // ipa_off >= 16 here
  }
  return ether_type;
}

// Indexed launches load the cooperative window blocks at the default cache policy (LWIN = 0): in a
// packed capture a frame's last line is the next frame's window line, and a block loaded
// with default policy is still in L2 when the previous frame's stream asks for it
// (packed C2/C3/C5 -8..-10 %, permuted ef_vi event runs -2 %, in-order slot runs +1 %;
// profiles/r01_experiments/indexed_window_policy_c{2,3,5}.json).
constexpr int kIdxWin = 0;

// Header window of this lane's frame for an indexed layout: the window (ip - MIS) at `win`, the frame's Ethernet
// header `o` bytes past the base and `avail` bytes long at most.  Lanes without `use` (past n, or an offset outside
// the launch's alignment class) read nothing and keep a zero window.  Returns the ether_type as stored.
// Every lane of the workgroup must call it: with COOP it ballots and meets two barriers.
// COOP = 1: when every used frame of the wave has its 128-B window block (the 16-B chunk before the window, and the
// window) 16-B aligned inside [base, eth + avail), 8 lanes per frame load the block coalesced into the LDS tile, as
// load_window_strided does (one request per line; the second line of a straddling block only when the header
// fields reach it), at the default cache policy for LWIN = 0, else non-temporal.  Other waves, and COOP = 0, load
// per lane: chunk c spans eth + (14 - MIS) + 16c .. +16 and is loaded whole when it lies inside avail; the one chunk
// avail ends in is read by the dwords that begin below avail (a segment or datagram may end in it, and the header
// lane sums the window below the stream start from these registers; an aligned dword lies in the page of its first
// byte).
template <int MIS, int COOP, int LWIN>
__device__ __forceinline__ uint32_t load_window_indexed(const uint8_t* win, uint64_t o, bool use, uint32_t avail,
                                                        int lane, Window& h) {
  uint32_t ether_type = 0;
#pragma unroll
  for (int q = 0; q < 4 * kWinChunks; ++q) h.d[q] = 0;
  bool coop = false; // wave-uniform
  if constexpr (COOP) {
    const bool elig = !use || ((((uintptr_t)win & 15u) == 0) && o + 14 >= (uint64_t)(MIS + 16) &&
                               (uint32_t)(14 - MIS + kWinBytes) <= avail);
    coop = __all(elig);
  }
  if (coop) {
    __shared__ uint64_t line_addr[kFramesPerWave];
    line_addr[lane] = use ? (uint64_t)(win - 16) : 0ull;
    __syncthreads();
    u32x4* tile = coop_tile();
    // all 8 loads in flight before the first LDS write (as load_window_strided): a part that is not
    // needed reads its block's first chunk instead -- a line the same instruction fetches anyway (or,
    // for an unused row, the first used frame's block) -- and is zeroed, rather than a branch around it
    const uint64_t used = __ballot(use);
    const uint32_t l0 = used ? (uint32_t)__builtin_ctzll(used) : 0u;
    const uint64_t wb = (uint64_t)(win - 16);
    const uint64_t safe = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(wb >> 32), l0) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((uint32_t)wb, l0);
    u32x4 v[8];
    bool need[8];
    const u32x4* src[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      const uint64_t la = line_addr[r];
      need[i] = la && block_part_needed<MIS>((uint32_t)la, part);
      src[i] = need[i] ? reinterpret_cast<const u32x4*>(la) + part : reinterpret_cast<const u32x4*>(la ? la : safe);
      v[i] = u32x4{0u, 0u, 0u, 0u};
    }
    if (used != 0) { // wave-uniform: a wave with no frame to classify loads nothing
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if constexpr (LWIN == 0) v[i] = *src[i];
        else v[i] = __builtin_nontemporal_load(src[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t r = 8 * i + (lane >> 3), part = lane & 7;
      tile[r * 8 + (part ^ (r & 7))] = need[i] ? v[i] : u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const u32x4 v = tile[lane * 8 + ((1 + c) ^ (lane & 7))];
      h.d[4 * c + 0] = v.x;
      h.d[4 * c + 1] = v.y;
      h.d[4 * c + 2] = v.z;
      h.d[4 * c + 3] = v.w;
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = tile[lane * 8 + (0 ^ (lane & 7))].w >> 16;
  } else if (use) {
    // a chunk past avail re-reads chunk 0 (a line this lane fetches anyway) and is dropped, rather than a branch
    // around its load, so the 7 loads are in flight together
    u32x4 v[kWinChunks];
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const bool in = (uint32_t)(14 - MIS + 16 * c + 16) <= avail;
      v[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(win) + (in ? c : 0));
    }
#pragma unroll
    for (int c = 0; c < kWinChunks; ++c) {
      const uint32_t lo = (uint32_t)(14 - MIS + 16 * c); // the chunk's first byte, relative to eth
      if (lo + 16 <= avail) {
        h.d[4 * c + 0] = v[c].x;
        h.d[4 * c + 1] = v[c].y;
        h.d[4 * c + 2] = v[c].z;
        h.d[4 * c + 3] = v[c].w;
      } else if (lo < avail) { // wave-uniform
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (lo + 4 * q < avail) h.d[4 * c + q] = reinterpret_cast<const uint32_t*>(win)[4 * c + q];
      }
    }
    if constexpr (MIS >= 2) ether_type = h.template u16<MIS - 2>();
    else ether_type = *reinterpret_cast<const uint32_t*>(win - 4) >> 16; // eth + 10 - MIS >= eth
  }
  return ether_type;
}

// Exact u16-word sum of the window's bytes in [lo, end) (lo compile-time, end even).
template <int LO>
__device__ __forceinline__ uint32_t window_sum_from(const Window& h, int end) {
  uint32_t t = 0;
#pragma unroll
  for (int q = LO / 4; q < 4 * kWinChunks; ++q) {
    const uint32_t start_sel = ((4 * q >= LO) ? 1u : 0u) | ((4 * q + 2 >= LO) ? 0x10000u : 0u);
    t = dot2(h.d[q], tail_sel(end, 4 * q) & start_sel, t);
  }
  return t;
}

// The header lane's share of the summed region [MIS, end): the window's words below the
// stream start s0; when s0 = 0 < MIS the stream also sums [0, MIS), taken back here.
template <int MIS>
__device__ __forceinline__ uint32_t window_part(const Window& h, int end, uint32_t s0) {
  uint32_t t = window_sum_from<MIS>(h, min(end, (int)s0));
  if constexpr (MIS > 0) {
    if (s0 == 0 && end > 0) t -= h.template sum16<0, MIS>();
  }
  return t;
}

// XCD-aware group order: workgroup b (dispatched to XCD b % 8) -> group index such that every
// XCD owns one contiguous eighth of the nwg groups (a bijection on [0, nwg)).
// Frames per wave for a batch of n (host side, at launch): 64 once the batch fills the chip
// (>= 1024 waves = 4 per CU), else halved down to 8, so a small batch (a poll's worth of RX
// events) runs on more waves with fewer dependent stream rounds each -- latency, not
// bandwidth, bounds those launches.
inline uint32_t frames_per_wave(uint32_t n) {
  uint32_t fpw = kFramesPerWave;
  while (fpw > 8 && (n + fpw - 1) / fpw < 1024) fpw >>= 1;
  return fpw;
}

// f(std::integral_constant<int, MIS>{}) for the alignment class MIS = (off + 14) % 16 of an even Ethernet-header
// offset: every launch of a kernel specialised on it (RX classify, TX fill) goes through here.
template <class F>
void for_mis(uint32_t off, F&& f) {
  switch ((off + 14) & 15) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return f(std::integral_constant<int, 14>{});
  }
}

// Completion word (pn_classify_notify / pn_tx_fill_notify): every workgroup makes its stores
// system-visible and counts itself done; the last one resets the device counter and stores
// `token` to the host-visible word, so a host polling the word sees the batch done without
// waiting for the launch's completion signal.  Each workgroup's system fence writes back L2,
// which is why the notify entry points are limited to small batches (PN_NOTIFY_MAX_FRAMES).
// Only vector memory operations (a global atomic, vector stores).
__device__ __forceinline__ void signal_done(uint32_t* count, uint32_t* word, uint32_t token, int lane) {
  __threadfence_system();
  if (lane == 0) {
    const uint32_t prev = atomicAdd(count, 1u);
    if (prev == gridDim.x - 1) {
      __threadfence_system();
      count[0] = 0u;
      __hip_atomic_store(word, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

__device__ __forceinline__ uint32_t xcd_group(uint32_t b, uint32_t nwg) {
  const uint32_t per = (nwg + 7) / 8, x = b % 8, k = b / 8;
  const uint32_t full = nwg % 8 == 0 ? 8 : nwg % 8; // XCDs that own `per` groups (the rest own per - 1)
  return x < full ? x * per + k : full * per + (x - full) * (per - 1) + k;
}

// Stream start of the window at w, relative to w: the first 128-B line boundary past the
// window's 16-B block start (w - 16).  112 (the window end) for the default layout, where the
// block is the slot's first line; less where the block straddles two lines, so the stream's
// 1-KiB loads still cover whole lines and no line is requested by two of them.  The header
// lane sums the window below it.  A multiple of 16 (word parity kept for any w).
__device__ __forceinline__ uint32_t stream_start(uint64_t w) { return 112u - (((uint32_t)w - 16u) & 112u); }

// ---- phase 2: the wave streams every frame's region from its stream start on ----
// group_ipa: window start of the group's first slot; frame fi's window is at
// group_ipa + fi*stride.  end_rel is this lane's frame extent (read back per
// frame with readlane); the total of frame fi lands on lane fi.  The header lane
// has summed the window below stream_start (window_part).
template <int ABL, int LAUX, int IDX>
__device__ __forceinline__ void stream_phase(uint32_t stride, const uint8_t* group_ipa, uint64_t my_win, uint32_t n_here,
                                             int lane, int end_rel, uint32_t& t_all, uint32_t& pad) {
  static_assert(ABL & kExactRange, "every frame's stream descriptor ends at its dword-exact extent");
  // window start of frame fi: strided from the group's first slot, or (indexed) the
  // address its own lane computed, broadcast with two readlanes
  auto frame_win = [&](uint32_t fi) -> const uint8_t* {
    if constexpr (IDX) {
      const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)my_win, fi & 63);
      const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(my_win >> 32), fi & 63);
      return (const uint8_t*)(((uint64_t)hi << 32) | lo);
    } else {
      return group_ipa + (uint64_t)fi * stride;
    }
  };
  for (uint32_t b0 = 0; b0 < n_here; b0 += kBatch) {
    uint32_t acc[kBatch];
    int ends[kBatch], s0s[kBatch];
    u32x4 w0s[kBatch], w1s[kBatch];
    // issue all 2*kBatch loads of the batch before consuming any of them
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const uint32_t fi = b0 + j; // wave-uniform
      const int end = __builtin_amdgcn_readlane(end_rel, fi & 63) & ~1; // bit 0 = odd tcp_len, read below
      ends[j] = end;
      const uint32_t end16 = (uint32_t)(end + 3) & ~3u; // dword-exact extent; 0 for frames past n (end_rel = 0 there)
      const uint8_t* fw = frame_win(fi);
      const int s0 = (int)stream_start((uint64_t)fw);
      s0s[j] = s0;
      const __amdgpu_buffer_rsrc_t rs = frame_rsrc(fw, end16);
      // out-of-range chunks of a buffer load return 0 and fetch nothing
      if constexpr (ABL & kSkipEmptyLoads) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        w0s[j] = end16 > (uint32_t)s0 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + lane * 16, 0, LAUX) : z;
        w1s[j] = end16 > (uint32_t)s0 + 1024 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + 1024 + lane * 16, 0, LAUX) : z;
      } else {
        w0s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + lane * 16, 0, LAUX);
        w1s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + 1024 + lane * 16, 0, LAUX);
      }
    }
    __builtin_amdgcn_sched_barrier(0); // keep the whole batch in flight before the first wait
    // Both halves of every dword count: the descriptor's exact range has zeroed what lies past the extent.  The
    // (extent, offset) arguments are what the per-dword tail masks took before kExactRange; writing the constant at
    // the call sites instead changes the code of 40 RX and 48 TX kernels (measured when the masks were removed), so
    // the lambda and its arguments stay until the kernels are next re-measured.
    auto sel = [](int, int) -> uint32_t { return 0x10001u; };
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int end = ends[j], s0 = s0s[j];
      const u32x4 w0 = w0s[j], w1 = w1s[j];
      const int o0 = s0 + lane * 16, o1 = o0 + 1024;
      uint32_t sum = 0;
      sum = dot2(w0.x, sel(end, o0), sum);
      sum = dot2(w0.y, sel(end, o0 + 4), sum);
      sum = dot2(w0.z, sel(end, o0 + 8), sum);
      sum = dot2(w0.w, sel(end, o0 + 12), sum);
      sum = dot2(w1.x, sel(end, o1), sum);
      sum = dot2(w1.y, sel(end, o1 + 4), sum);
      sum = dot2(w1.z, sel(end, o1 + 8), sum);
      sum = dot2(w1.w, sel(end, o1 + 12), sum);
      // end % 4 == 2: the last dword loaded holds the 2 bytes after the extent (its high half)
      const int q2 = end - 2 - s0; // wave-uniform
      if ((end & 2) && q2 >= 0 && q2 < 2048) {
        const u32x4 w = (q2 < 1024) ? w0 : w1;
        const int dw = (q2 >> 2) & 3;
        const uint32_t d = dw == 0 ? w.x : dw == 1 ? w.y : dw == 2 ? w.z : w.w;
        if (lane == ((q2 & 1023) >> 4)) sum -= d >> 16;
      }
      acc[j] = sum;
      // odd tcp_len: the RFC verdict needs the byte the reference sums past the segment (window
      // offset end - 1); take it from the lane that streamed it instead of re-reading the line later
      const int p = end - 1;
      if ((__builtin_amdgcn_readlane(end_rel, (b0 + j) & 63) & 1) && p >= s0 && p < s0 + 2048) {
        const int q = p - s0;                        // wave-uniform
        const u32x4 w = (q < 1024) ? w0 : w1;
        const int dw = (q >> 2) & 3;
        const uint32_t d = dw == 0 ? w.x : dw == 1 ? w.y : dw == 2 ? w.z : w.w;
        const uint32_t b = __builtin_amdgcn_readlane((d >> (8 * (q & 3))) & 0xff, (q & 1023) >> 4);
        if ((uint32_t)lane == b0 + j) pad = b;
      }
    }
    // jumbo slots only (slot_stride > 2048): KiBs past the two streamed above, wave-uniform
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int end = ends[j], s0 = s0s[j];
      if (end > s0 + 2048) {
        const __amdgpu_buffer_rsrc_t rs = frame_rsrc(frame_win(b0 + j), (uint32_t)(end + 15) & ~15u);
        uint32_t sum = acc[j];
        for (int kb = s0 + 2048; kb < end; kb += 1024) {
          const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, kb + lane * 16, 0, LAUX);
          const int o = kb + lane * 16;
          sum = dot2(w.x, tail_sel(end, o), sum);
          sum = dot2(w.y, tail_sel(end, o + 4), sum);
          sum = dot2(w.z, tail_sel(end, o + 8), sum);
          sum = dot2(w.w, tail_sel(end, o + 12), sum);
        }
        acc[j] = sum;
      }
    }
    // transpose-reduce 8 frames x 64 lanes: lane l ends with the total of frame (l>>3)&7
    if constexpr (ABL & kAblNoReduce) {
      uint32_t x = 0;
#pragma unroll
      for (int j = 0; j < kBatch; ++j) x += acc[j];
      if ((uint32_t)(lane >> 3) == b0 / kBatch) t_all += x;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { // xor 32: v_permlane32_swap
        const auto r = __builtin_amdgcn_permlane32_swap(acc[i], acc[i + 4], false, false);
        acc[i] = r[0] + r[1];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) { // xor 16: v_permlane16_swap
        const auto r = __builtin_amdgcn_permlane16_swap(acc[i], acc[i + 2], false, false);
        acc[i] = r[0] + r[1];
      }
      const bool b3 = lane & 8; // xor 8: keep one, send the other
      const uint32_t keep = b3 ? acc[1] : acc[0];
      const uint32_t send = b3 ? acc[0] : acc[1];
      uint32_t v = keep + dpp<0x128>(send); // row_ror:8           -> lane ^ 8
      v += dpp<0xB1>(v);                    // quad_perm [1,0,3,2]  -> lane ^ 1
      v += dpp<0x4E>(v);                    // quad_perm [2,3,0,1]  -> lane ^ 2
      v += dpp<0x141>(v);                   // row_half_mirror      -> other quad of the 8
      const uint32_t tot = __shfl(v, (lane & 7) * 8);
      if ((uint32_t)(lane >> 3) == b0 / kBatch) t_all += tot;
    }
  }
}

// Phase 2 software-pipelined by half batches (kPipeStream; strides up to 2048, where no frame reaches
// past its two stream KiBs, and every load issued): the next half's 8 loads go out before the current
// half is summed, so a wave always has 8-16 loads in flight instead of draining to none at each batch
// boundary.  Same loads, same sums, same reduction as stream_phase.
template <int ABL, int LAUX, int IDX>
__device__ __forceinline__ void stream_phase_pipelined(uint32_t stride, const uint8_t* group_ipa, uint64_t my_win,
                                                       uint32_t n_here, int lane, int end_rel, uint32_t& t_all,
                                                       uint32_t& pad) {
  static_assert(!(ABL & kSkipEmptyLoads) && (ABL & kExactRange), "pipelined phase 2: every load issued, exact ranges");
  constexpr int kHalf = kBatch / 2;
  auto frame_win = [&](uint32_t fi) -> const uint8_t* {
    if constexpr (IDX) {
      const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)my_win, fi & 63);
      const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(my_win >> 32), fi & 63);
      return (const uint8_t*)(((uint64_t)hi << 32) | lo);
    } else {
      return group_ipa + (uint64_t)fi * stride;
    }
  };
  int ends[kBatch], s0s[kBatch];
  u32x4 w0s[kBatch], w1s[kBatch];
  uint32_t acc[kBatch];
  // the loads of frames fi0 .. fi0+3 into slots j0 .. j0+3 (frames past n_here: end_rel 0, nothing fetched)
  auto issue = [&](uint32_t fi0, int j0) {
#pragma unroll
    for (int q = 0; q < kHalf; ++q) {
      const int j = j0 + q;
      const uint32_t fi = fi0 + q; // wave-uniform
      // past the wave's frames (the last batch's look-ahead): an empty range, the load fetches nothing
      const int end = fi < n_here ? __builtin_amdgcn_readlane(end_rel, fi & 63) & ~1 : 0;
      ends[j] = end;
      const uint32_t end16 = (uint32_t)(end + 3) & ~3u;
      const uint8_t* fw = frame_win(fi);
      const int s0 = (int)stream_start((uint64_t)fw);
      s0s[j] = s0;
      const __amdgpu_buffer_rsrc_t rs = frame_rsrc(fw, end16);
      w0s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + lane * 16, 0, LAUX);
      w1s[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, s0 + 1024 + lane * 16, 0, LAUX);
    }
  };
  // sum slots j0 .. j0+3 (frames fi0 ..) into acc, with the 2-mod-4 correction and the odd-length pad byte
  auto consume = [&](uint32_t fi0, int j0) {
#pragma unroll
    for (int q = 0; q < kHalf; ++q) {
      const int j = j0 + q;
      const int end = ends[j], s0 = s0s[j];
      const u32x4 w0 = w0s[j], w1 = w1s[j];
      uint32_t sum = 0;
      sum = dot2(w0.x, 0x10001u, sum);
      sum = dot2(w0.y, 0x10001u, sum);
      sum = dot2(w0.z, 0x10001u, sum);
      sum = dot2(w0.w, 0x10001u, sum);
      sum = dot2(w1.x, 0x10001u, sum);
      sum = dot2(w1.y, 0x10001u, sum);
      sum = dot2(w1.z, 0x10001u, sum);
      sum = dot2(w1.w, 0x10001u, sum);
      const int q2 = end - 2 - s0; // wave-uniform
      if ((end & 2) && q2 >= 0 && q2 < 2048) {
        const u32x4 w = (q2 < 1024) ? w0 : w1;
        const int dw = (q2 >> 2) & 3;
        const uint32_t d = dw == 0 ? w.x : dw == 1 ? w.y : dw == 2 ? w.z : w.w;
        if (lane == ((q2 & 1023) >> 4)) sum -= d >> 16;
      }
      acc[j] = sum;
      const int p = end - 1;
      if ((__builtin_amdgcn_readlane(end_rel, (fi0 + q) & 63) & 1) && p >= s0 && p < s0 + 2048) {
        const int qq = p - s0;
        const u32x4 w = (qq < 1024) ? w0 : w1;
        const int dw = (qq >> 2) & 3;
        const uint32_t d = dw == 0 ? w.x : dw == 1 ? w.y : dw == 2 ? w.z : w.w;
        const uint32_t b = __builtin_amdgcn_readlane((d >> (8 * (qq & 3))) & 0xff, (qq & 1023) >> 4);
        if ((uint32_t)lane == fi0 + q) pad = b;
      }
    }
  };
  issue(0, 0);
  for (uint32_t b0 = 0; b0 < n_here; b0 += kBatch) {
    issue(b0 + kHalf, kHalf);
    consume(b0, 0);
    // the next batch's first half, under this one's second.  Unconditional (past the last batch its
    // ranges are empty): behind a branch the compiler could no longer count the loads in flight and
    // would wait for them before summing this batch's second half.
    issue(b0 + kBatch, 0);
    consume(b0 + kHalf, kHalf);
    if constexpr (ABL & kAblNoReduce) { // timing only (the ablated ceiling kernel), as stream_phase
      uint32_t x = 0;
#pragma unroll
      for (int j = 0; j < kBatch; ++j) x += acc[j];
      if ((uint32_t)(lane >> 3) == b0 / kBatch) t_all += x;
      continue;
    }
    // transpose-reduce 8 frames x 64 lanes as stream_phase: lane l ends with the total of frame (l>>3)&7
    uint32_t r8[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) r8[i] = acc[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const auto r = __builtin_amdgcn_permlane32_swap(r8[i], r8[i + 4], false, false);
      r8[i] = r[0] + r[1];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const auto r = __builtin_amdgcn_permlane16_swap(r8[i], r8[i + 2], false, false);
      r8[i] = r[0] + r[1];
    }
    const bool b3 = lane & 8;
    const uint32_t keep = b3 ? r8[1] : r8[0];
    const uint32_t send = b3 ? r8[0] : r8[1];
    uint32_t v = keep + dpp<0x128>(send);
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    const uint32_t tot = __shfl(v, (lane & 7) * 8);
    if ((uint32_t)(lane >> 3) == b0 / kBatch) t_all += tot;
  }
}

} // namespace pn_dev
