// The layouts of wide_layout.hpp against the expressions their users wrote out by hand before the header
// existed (tests/test_accel_layout.py).  Prints "ok <cases>" or the first difference.
#include <cstdio>
#include <cstdlib>

#include "../../raytracercpp_amd/csrc/wide_layout.hpp"

static int cases = 0;

static void eq(const char* what, size_t nn, size_t nt, size_t got, size_t want)
{
    cases++;
    if (got == want)
        return;
    printf("FAIL %s(nn=%zu, nt=%zu) = %zu, expected %zu\n", what, nn, nt, got, want);
    exit(1);
}

int main()
{
    using namespace rt;
    static_assert(wide_risk_bytes(7) == 7 * 288 + 64 && wide_links_parent_off(7, 5) == 20, "constexpr");
    const size_t NN[4] = {1, 2, 7, 4096}, NT[3] = {1, 3, 5};
    for (size_t nn : NN)
        for (size_t nt : NT) {
            eq("wide_risk_bytes", nn, nt, wide_risk_bytes(nn), nn * 288 + 64);
            eq("wide_risk_words_off", nn, nt, wide_risk_words_off(nn), 0);
            eq("wide_risk_keys_off", nn, nt, wide_risk_keys_off(nn), nn * 64);
            eq("wide_risk_boxes_off", nn, nt, wide_risk_boxes_off(nn), nn * 96);
            eq("wide_risk_caps_off", nn, nt, wide_risk_caps_off(nn), nn * 288);
            // every region aligned to its element: 8-B words, 4-B keys, floats and caps
            eq("words % 8", nn, nt, wide_risk_words_off(nn) % 8, 0);
            eq("keys % 4", nn, nt, wide_risk_keys_off(nn) % 4, 0);
            eq("boxes % 4", nn, nt, wide_risk_boxes_off(nn) % 4, 0);
            eq("caps % 4", nn, nt, wide_risk_caps_off(nn) % 4, 0);
            // the typed pointers are the same offsets from the base
            alignas(8) static char base[4096 * 288 + 64];
            const WRiskView R = wide_risk_view(base, nn);
            eq("view.words", nn, nt, (size_t)((char*)R.words - base), 0);
            eq("view.keys", nn, nt, (size_t)((char*)R.keys - base), nn * 64);
            eq("view.boxes", nn, nt, (size_t)((char*)R.boxes - base), nn * 96);
            eq("view.caps", nn, nt, (size_t)((char*)R.caps - base), nn * 288);
            eq("view.entries", nn, nt, R.entries, nn * 8);
            eq("wide_tmp_slot_off", nn, nt, wide_tmp_slot_off(nn, nt), 0);
            eq("wide_tmp_leaf_of_slot_off", nn, nt, wide_tmp_leaf_of_slot_off(nn, nt), nt * 4);
            eq("wide_tmp_bytes", nn, nt, wide_tmp_bytes(nn, nt), nt * 8);
            eq("wide_links_tri_leaf_off", nn, nt, wide_links_tri_leaf_off(nn, nt), 0);
            eq("wide_links_parent_off", nn, nt, wide_links_parent_off(nn, nt), nt * 4);
            eq("wide_links_bytes", nn, nt, wide_links_bytes(nn, nt), (nt + nn) * 4);
        }
    printf("ok %d\n", cases);
    return 0;
}
