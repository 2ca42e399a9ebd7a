// Host check of loma-nerf_amd/csrc/lnerf_wave_addr.h: the split "wave-uniform base + per-lane
// constant (+ immediate)" that k1 and kr hand to the SGPR-base forms of the LDS-DMA and of the slab
// stores, against the pointer expressions the kernels used before the split, for every lane; every
// address inside its chunk, ring slot or slab; every byte of a chunk and of a slab written exactly
// once. Built and run by tests/test_wave_addr.py (host compiler, -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lnerf_wave_addr.h"

using namespace lnerf::waddr;

static int g_fail = 0;
#define CHECK(c, ...)                                 \
    do {                                              \
        if (!(c)) {                                   \
            if (g_fail++ < 20) {                      \
                std::printf("FAIL %s: ", #c);         \
                std::printf(__VA_ARGS__);             \
                std::printf("\n");                    \
            }                                         \
        }                                             \
    } while (0)

// ---- LDS-DMA pieces of one chunk: NW waves, `bytes` long, into a ring slot of slot_bytes at LDS
// address `slot`; the chunk is the last one of a weight buffer that ends at src + bytes.
static long check_chunk(int nw, int bytes, uint32_t slot, int slot_bytes, bool* uneven) {
    const uint64_t src = 0x7f3a00001000ull + (uint64_t)bytes * 3;   // a device address (never dereferenced)
    std::vector<unsigned char> src_hit(bytes, 0), lds_hit(slot_bytes, 0);
    long pieces = 0;
    int nmin = 1 << 30, nmax = 0;
    for (int wave = 0; wave < nw; ++wave) {
        // the count as the kernels computed it
        const int woff = wave * 1024;
        const int n_old = woff < bytes ? (bytes - woff + nw * 1024 - 1) / (nw * 1024) : 0;
        const int n = dma_piece_count(bytes, wave, nw);
        CHECK(n == n_old, "pieces nw %d bytes %d wave %d: %d vs %d", nw, bytes, wave, n, n_old);
        nmin = n < nmin ? n : nmin;
        nmax = n > nmax ? n : nmax;
        // the job's scalars: the wave's piece 0 at both ends
        const uint64_t job_src = src + dma_wave_off(wave);
        const uint32_t job_dst = slot + dma_wave_off(wave);
        for (int p = 0; p < n; ++p, ++pieces) {
            const uint64_t sbase = job_src + dma_piece_off(p, nw);   // scalar pair
            const uint32_t m0 = job_dst + dma_piece_off(p, nw);      // scalar, into M0
            for (int lane = 0; lane < 64; ++lane) {
                const uint64_t addr = sbase + dma_lane_off(lane);    // + the one vector operand
                const uint64_t old_addr = src + (uint64_t)woff + (uint64_t)p * (nw * 1024) + (uint64_t)lane * 16;
                CHECK(addr == old_addr, "src nw %d bytes %d wave %d p %d lane %d", nw, bytes, wave, p, lane);
                CHECK(addr >= src && addr + 16 <= src + (uint64_t)bytes, "src range nw %d bytes %d wave %d p %d lane %d",
                      nw, bytes, wave, p, lane);
                // the hardware writes lane-linear from M0
                const uint32_t l = m0 + (uint32_t)lane * 16;
                const uint32_t old_l = slot + (uint32_t)woff + (uint32_t)p * (nw * 1024) + (uint32_t)lane * 16;
                CHECK(l == old_l, "lds nw %d bytes %d wave %d p %d lane %d", nw, bytes, wave, p, lane);
                CHECK(l >= slot && l + 16 <= slot + (uint32_t)slot_bytes, "lds range nw %d bytes %d wave %d p %d", nw,
                      bytes, wave, p);
                CHECK(l - slot == addr - src, "both ends at the same chunk offset");
                if (addr >= src && addr + 16 <= src + (uint64_t)bytes)
                    for (int b = 0; b < 16; ++b) {
                        ++src_hit[addr - src + b];
                        ++lds_hit[l - slot + b];
                    }
            }
        }
    }
    for (int b = 0; b < bytes; ++b) CHECK(src_hit[b] == 1 && lds_hit[b] == 1, "chunk byte %d of %d (nw %d) moved %d times", b, bytes, nw, src_hit[b]);
    for (int b = bytes; b < slot_bytes; ++b) CHECK(lds_hit[b] == 0, "slot byte %d past the chunk written", b);
    if (nmin != nmax) *uneven = true;
    return pieces;
}

// ---- slab stores of one layer: nblk 32-sample blocks x kt k-steps; a block holds, per k-step, the
// two waves' half-block runs, each two feature halves of [16 samples][16 features].
template <bool I24>
static void check_slab(int nblk, int kt) {
    const int esz = I24 ? 3 : 4;                 // bytes per value
    const uint64_t at = 1024ull * esz;           // one k-step of one block: 32 samples x 32 features
    const uint64_t base = 0x7f5b00000400ull;     // the layer's slab (never dereferenced)
    const uint64_t size = (uint64_t)nblk * kt * at;
    std::vector<unsigned char> hit(size, 0);
    const int per_lane = 4 * esz;                // 4 values per lane and store
    for (int blk = 0; blk < nblk; ++blk)         // (the last block of the layer included)
        for (int half = 0; half < 2; ++half) {
            // the wave's run of this pass (k16_fwd_bwd_kernel: slab[q])
            const uint64_t slab = base + (uint64_t)blk * kt * at + (uint64_t)half * (at / 2);
            for (int s = 0; s < 8 && s < kt; ++s) {
                const uint64_t sbase = slab + (I24 ? slab_step_off_24(s) : slab_step_off_f32(s));   // scalar pair
                for (int h = 0; h < 2; ++h) {
                    const uint32_t imm = h * (I24 ? kSlabHalf24 : kSlabHalfF32);                 // instruction offset
                    CHECK(imm < 4096, "the feature half fits the 13-bit signed instruction offset");
                    for (int lane = 0; lane < 64; ++lane) {
                        const int n = lane & 15, g = lane >> 4;
                        const uint64_t addr = sbase + (I24 ? slab_lane_off_24(lane) : slab_lane_off_f32(lane)) + imm;
                        // the expressions before the split: float* dst = slab + s * 1024 (floats),
                        // dst + n * 16 + 4 * g, dst + 256 + ...; bytes dst = slab + s * 3072,
                        // dst + n * 48 + 12 * g, dst + 768 + ...
                        const uint64_t old_addr = I24 ? slab + (uint64_t)s * 3072 + (h ? 768 : 0) + n * 48 + 12 * g
                                                      : slab + 4 * ((uint64_t)s * 1024 + (h ? 256 : 0) + n * 16 + 4 * g);
                        CHECK(addr == old_addr, "slab i24 %d blk %d half %d s %d h %d lane %d", (int)I24, blk, half, s, h,
                              lane);
                        CHECK(addr % 4 == 0, "4-byte aligned");
                        const bool in = addr >= base && addr + per_lane <= base + size;
                        CHECK(in, "slab range i24 %d blk %d/%d half %d s %d h %d lane %d", (int)I24, blk, nblk, half, s, h,
                              lane);
                        if (in)
                            for (int b = 0; b < per_lane; ++b) ++hit[addr - base + b];
                    }
                }
            }
        }
    // no byte is written twice, and the stores cover what the pass holds (all of the layer when
    // kt <= 8)
    long twice = 0, total = 0;
    for (uint64_t b = 0; b < size; ++b) {
        twice += hit[b] > 1;
        total += hit[b];
    }
    CHECK(twice == 0, "i24 %d nblk %d kt %d: %ld bytes written twice", (int)I24, nblk, kt, twice);
    CHECK(total == (long)nblk * 2 * (kt < 8 ? kt : 8) * 2 * 64 * per_lane, "i24 %d: bytes stored", (int)I24);
}

int main() {
    long pieces = 0;
    bool uneven = false;
    // NW = 8: 64 KiB slots (fp16x3 / bf16), 48 KiB (bf16x6, KC = 1); NW = 4: 32 KiB slots. Every
    // chunk length from 1 KiB to the slot: whole chunks, and partial ones where bytes is no multiple
    // of NW KiB, so that the waves issue different numbers of pieces (or none).
    const struct { int nw, slot_bytes; uint32_t slot; } rings[] = {
        {8, 65536, 0}, {8, 65536, 65536}, {8, 49152, 2 * 49152}, {4, 32768, 32768}, {8, 32768, 2 * 32768}};
    for (const auto& r : rings)
        for (int kib = 1; kib * 1024 <= r.slot_bytes; ++kib) pieces += check_chunk(r.nw, kib * 1024, r.slot, r.slot_bytes, &uneven);
    CHECK(uneven, "some partial chunk gives the waves different piece counts");
    CHECK(dma_piece_count(65536, 7, 8) == 8 && dma_piece_count(32768, 3, 4) == 8, "a whole chunk is 8 pieces per wave");
    // slabs: all 8 k-steps, both halves, every block up to the layer's last; ragged layers (kt < 8)
    for (int kt : {1, 2, 3, 8})
        for (int nblk : {1, 5}) {
            check_slab<false>(nblk, kt);
            check_slab<true>(nblk, kt);
        }
    if (g_fail) {
        std::printf("%d address checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all wave address checks passed (%ld DMA pieces)\n", pieces);
    return 0;
}
