// Host-side check of the per-wave table of the ring kernel (rwkv.cpp_amd/csrc/ring_geom.h, rg_wave), compiled and run by
// tests/test_ring_wave_table.py: every entry equals what the rg_* functions give for that workgroup, consumer wave and phase, and the
// ring offsets the kernel derives from it without a division (ring_v6.hip, pre_begin: layer offset modulo the ring + the entry's offset
// modulo the ring, one conditional subtraction) are the stream positions modulo the ring size, layer after layer. No GPU, no HIP headers.
#include "ring_geom.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace rwkvmi;

static int fails = 0;
#define CHECK(COND, ...) do { if (!(COND)) { fails++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); if (fails > 20) exit(1); } } while (0)

static void check_shape(const RingShape & s, uint32_t ring, int n_layers, const char * name) {
    for (int b = 0; b < RG_NBLK; b++) {
        const RingCu cu = rg_cu(s, b);
        for (int c = 0; c < RG_NC; c++) {
            const RingWave w = rg_wave(cu, c, ring);
            CHECK(rg_wave_index(b, c) == b * RG_NC + c, "%s: index", name);
            CHECK(w.layer_bytes == cu.layer_bytes && w.layer_ro == cu.layer_bytes % ring, "%s wg %d wave %d: layer bytes", name, b, c);
            CHECK(w.first_own == rg_next_own_in_layer(cu, c, 0), "%s wg %d wave %d: first own record", name, b, c);
            for (int ph = 0; ph < RG_NPHASE; ph++) {
                const RingWavePhase & e = w.ph[ph];
                CHECK(e.j0 == rg_first_j(cu, ph, c), "%s wg %d wave %d phase %d: j0", name, b, c, ph);
                CHECK(e.cnt == rg_own_count(cu, ph, c), "%s wg %d wave %d phase %d: count", name, b, c, ph);
                CHECK(e.pos == cu.off[ph] + rg_first_j(cu, ph, c) * cu.rec[ph], "%s wg %d wave %d phase %d: position", name, b, c, ph);
                CHECK(e.after == rg_next_own_in_layer(cu, c, ph + 1), "%s wg %d wave %d phase %d: after", name, b, c, ph);
                CHECK(e.ro == e.pos % ring && e.ro < ring, "%s wg %d wave %d phase %d: ring offset", name, b, c, ph);
                for (uint32_t t = 0; t < e.cnt; t++)
                    CHECK(e.j0 + RG_NC * t == rg_own_j(cu, ph, c, (int) t), "%s wg %d wave %d phase %d: record %u is not six apart", name, b, c, ph, t);
                // a wave that owns records of the phase: the first one is where the table says, inside the phase
                if (e.cnt) CHECK(e.j0 < cu.n[ph] && e.pos + cu.rec[ph] <= cu.layer_bytes, "%s wg %d wave %d phase %d: first record outside the block", name, b, c, ph);
            }
            // the kernel's cursors over the layers of a launch: lbase += layer_bytes, lro += layer_ro (mod ring), ro = lro + e.ro (mod ring)
            uint32_t lbase = 0, lro = 0;
            for (int li = 0; li < n_layers; li++) {
                for (int ph = 0; ph < RG_NPHASE; ph++) {
                    uint32_t ro = lro + w.ph[ph].ro;
                    ro = ro >= ring ? ro - ring : ro;
                    CHECK(ro == (lbase + w.ph[ph].pos) % ring, "%s wg %d wave %d layer %d phase %d: ring offset %u", name, b, c, li, ph, ro);
                }
                lbase += w.layer_bytes;
                lro += w.layer_ro; lro = lro >= ring ? lro - ring : lro;
            }
        }
    }
}

int main() {
    struct Fmt { const char * name; int qs, scb, qhb; } fmts[] = {{"Q4_0", 16, 2, 0}, {"Q4_1", 16, 4, 0}, {"Q5_0", 16, 2, 4}, {"Q5_1", 16, 4, 4}, {"Q8_0", 32, 2, 0}};
    const uint32_t rings[] = {32 * 1024, 76 * 1024, 100 * 1024, 116 * 1024};   // multiples of 4 KiB, as the host sizes the ring
    // every shape the device admits (ring_v6.hip, ring_variant -> rg_variant_key): 64 + 21 + 32 (D, F) pairs, both mix ranks
    const struct { int D, DR, want; } geos[] = {{2048, 64, 64}, {2560, 64, 21}, {4096, 128, 32}};
    int pairs = 0;
    for (const auto & g : geos) {
        int n = 0;
        for (int F = 32; F <= 20000; F += 32) {
            const bool in32 = rg_variant_key(g.D, F, g.DR, 32) >= 0, in64 = rg_variant_key(g.D, F, g.DR, 64) >= 0;
            CHECK(in32 == in64, "D %d F %d: the mix rank decides", g.D, F);
            if (!in32) continue;
            n++;
            for (int R : {32, 64})
                for (const Fmt & f : fmts)
                    for (uint32_t ring : rings) {
                        RingShape s; s.D = g.D; s.F = F; s.R5 = 5 * R; s.DR = g.DR; s.qs = f.qs; s.scb = f.scb; s.qhb = f.qhb;
                        char name[64]; snprintf(name, sizeof name, "%s D=%d F=%d R=%d ring=%u", f.name, g.D, F, R, ring);
                        check_shape(s, ring, 32, name);
                    }
        }
        CHECK(n == g.want, "D %d: %d admitted F, expected %d", g.D, n, g.want);
        pairs += n;
    }
    CHECK(pairs == 117, "%d admitted (D, F) pairs, expected 117", pairs);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    printf("ring wave table OK (%d admitted (D, F) pairs)\n", pairs);
    return 0;
}
