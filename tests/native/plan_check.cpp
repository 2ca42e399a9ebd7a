// plan_check.cpp -- the fused workspace's carve (loma-nerf_amd/csrc/lnerf_plan.h) on the host, for
// every combination of layer count, widths, batch, tile, slab format, train / render and dW budget
// that takes a different path through make_layout / fused_carve. Built with the host compiler under
// AddressSanitizer + UBSan (tests/test_plan.py); no HIP.
//
// Checked per carve: 64-float alignment, the regions' order, each region's room against what the
// layout says its user addresses (so the regions are pairwise disjoint and inside total), 16-byte
// aligned weight planes. Per shape: the a_tile = 768 and a_tile = 1024 carves share every offset but
// total with act last (the floor guard's sharing rule), every total is within the sizing value
// (fused_workspace_floats), the render carve is within the training carve and advances nothing for
// the training-only regions.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lnerf_plan.h"

using namespace lnerf;

namespace {

long long g_carves = 0;

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            fprintf(stderr, "plan_check: %s failed at line %d: %s\n", #cond, __LINE__, g_case);          \
            exit(1);                                                                                      \
        }                                                                                                 \
    } while (0)

char g_case[256];

constexpr int kRegions = 18;
struct Region {
    const char* name;
    size_t off, need;
};

// the regions in carve order, with the floats each one's user addresses (from the layout, stated
// here independently of fused_carve)
std::vector<Region> regions(const FusedCarve& c, const Layout& y, int L, int tile, bool train) {
    const size_t w16 = (y.w16_total + 1) / 2;
    return {
        {"guard", c.guard, 1},
        {"grad", c.grad, y.grad_total},
        {"loss_part", c.loss_part, (size_t)y.num_wg},
        {"dw_part", c.dw_part, y.dwp_total},
        {"db_part", c.db_part, y.dbp_total},
        {"loss_total", c.loss_total, 1},
        {"loss_stage", c.loss_stage, (size_t)kLossStage1},
        {"w16", c.w16, w16},
        {"w16x", c.w16x, w16},
        {"b16", c.b16, y.b16_total},
        {"mask_g", c.mask_g, y.mask_total * 2},
        {"wexp16", c.wexp16, (size_t)2 * kMaxLayers},   // wexp16, then dw_shift
        {"wmax_part", c.wmax_part, (size_t)kMaxLayers * kWmaxParts + (size_t)kWmaxParts * kHeadCols},
        {"hexp16", c.hexp16, (size_t)kHeadCols},
        {"sexp", c.sexp, train ? (size_t)L * y.num_wg * tile : 0},
        {"epart", c.epart, train ? (size_t)L * y.num_wg * (tile / 16) : 0},   // one per wave
        {"xcount", c.xcount, train ? (size_t)2 * y.dw_grid : 0},
        {"act", c.act, y.act_total},
    };
}

FusedCarve carve_of(const lnerf_mlp& m, int rays, int S, bool train, int dw_grid, int tile, int a_tile, Layout& y) {
    make_layout(y, m, rays, S, train, dw_grid, tile, a_tile);
    const FusedCarve c = fused_carve(y, m.num_layers, tile, train);
    const std::vector<Region> r = regions(c, y, m.num_layers, tile, train);
    CHECK((int)r.size() == kRegions);
    CHECK(r[0].off == 0);
    for (int i = 0; i < kRegions; ++i) {
        const size_t end = i + 1 < kRegions ? r[i + 1].off : c.total;
        CHECK(r[i].off % 64 == 0);
        CHECK(r[i].off <= end);                  // carve order: region i ends where region i + 1 starts,
        CHECK(r[i].need <= end - r[i].off);      // so room for its user makes the regions disjoint
        CHECK(end <= c.total);
    }
    CHECK(c.total % 64 == 0);
    CHECK(c.w16 * sizeof(float) % 16 == 0 && c.w16x * sizeof(float) % 16 == 0);
    // the layout's own offsets stay inside their regions
    for (int l = 0; l < m.num_layers; ++l) {
        CHECK(y.w16f_off[l] <= y.w16_total && y.w16b_off[l] <= y.w16_total);
        CHECK(y.w16f_off[l] % 8 == 0 && y.w16b_off[l] % 8 == 0);   // u16: 16-byte aligned planes
        if (train) {
            CHECK(y.grad_off[l] <= y.grad_total && y.dwp_off[l] <= y.dwp_total && y.dbp_off[l] <= y.dbp_total);
            if (l < m.num_layers - 1) CHECK(y.act_off[l] <= y.act_total);
            CHECK(y.splits[l] >= 1 && y.wg_off[l] + y.splits[l] <= y.dw_grid);
        }
    }
    ++g_carves;
    return c;
}

void check_shape(const lnerf_mlp& m, int rays, int S, int dw_grid) {
    const size_t sized[2] = {fused_workspace_floats(m, rays, S, false, dw_grid),
                             fused_workspace_floats(m, rays, S, true, dw_grid)};
    CHECK(sized[0] <= sized[1]);
    for (int tile = 128; tile >= (S <= 64 ? 64 : 128); tile /= 2) {
        FusedCarve c[2][2];   // [train][a_tile = 1024]
        Layout y;
        for (int train = 0; train < 2; ++train)
            for (int wide = 0; wide < 2; ++wide) {
                snprintf(g_case, sizeof g_case, "L %d k0 %d n0 %d rays %d S %d dw_grid %d tile %d train %d a_tile %d",
                         m.num_layers, m.k[0], m.n[0], rays, S, dw_grid, tile, train, wide ? 1024 : 768);
                c[train][wide] = carve_of(m, rays, S, train != 0, dw_grid, tile, wide ? 1024 : 768, y);
                CHECK(c[train][wide].total <= sized[train]);
            }
        for (int train = 0; train < 2; ++train) {
            // the floor guard's sharing rule: the fp16x3 plan (768) and its bf16x6 re-run (1024) differ
            // in nothing but where the last region, act, ends
            FusedCarve a = c[train][0], b = c[train][1];
            CHECK(a.total <= b.total);
            a.total = b.total = 0;
            const size_t* pa = &a.guard;
            const size_t* pb = &b.guard;
            for (int i = 0; i < kRegions; ++i) {
                CHECK(pa[i] == pb[i]);
                CHECK(pa[i] <= a.act);   // act is the last region
            }
        }
        for (int wide = 0; wide < 2; ++wide) {
            const FusedCarve& r = c[0][wide];
            CHECK(r.total <= c[1][wide].total);
            // a render carve: no slabs, no partials, no masks, no training-only words
            CHECK(r.loss_part == r.grad && r.db_part == r.dw_part && r.loss_total == r.db_part);
            CHECK(r.wexp16 == r.mask_g);
            CHECK(r.epart == r.sexp && r.xcount == r.sexp && r.act == r.sexp && r.total == r.sexp);
        }
    }
}

lnerf_mlp make_mlp(const std::vector<int>& widths) {   // widths: k[0], hidden ...; the head is 4 wide
    lnerf_mlp m{};
    m.num_layers = (int)widths.size();
    for (int l = 0; l < m.num_layers; ++l) {
        m.k[l] = widths[l];
        m.n[l] = l + 1 < m.num_layers ? widths[l + 1] : 4;
        m.w_k = m.k[l] > m.w_k ? m.k[l] : m.w_k;
        m.w_n = m.n[l] > m.w_n ? m.n[l] : m.w_n;
    }
    return m;
}

}  // namespace

int main() {
    static_assert(sizeof(FusedCarve) == (kRegions + 1) * sizeof(size_t), "one offset per region, then total");
    const int Ls[] = {1, 2, 8, 16}, W[] = {1, 4, 30, 33, 100, 256};
    const int rays[] = {1, 3, 129, 4096}, Ss[] = {1, 7, 30, 64, 128}, grids[] = {0, 16, 512, 4096};
    long long shapes = 0;
    for (int L : Ls) {
        // width vectors: every uniform one (all-256 among them), and rotations of the width list so that
        // each width meets each position and each neighbour
        std::vector<std::vector<int>> sets;
        for (int w : W) sets.push_back(std::vector<int>(L, w));
        for (int r = 0; r < 6; ++r) {
            std::vector<int> up(L), down(L);
            for (int l = 0; l < L; ++l) {
                up[l] = W[(r + l) % 6];
                down[l] = W[(r + 5 * l) % 6];
            }
            sets.push_back(up);
            sets.push_back(down);
        }
        for (const auto& widths : sets) {
            const lnerf_mlp m = make_mlp(widths);
            for (int n : rays)
                for (int S : Ss)
                    for (int g : grids) {
                        check_shape(m, n, S, g);
                        ++shapes;
                    }
        }
    }
    printf("all plan checks passed (%lld shapes, %lld carves)\n", shapes, g_carves);
    return 0;
}
