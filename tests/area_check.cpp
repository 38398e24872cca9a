// area_check.cpp -- resizes images with csrc/vstab_area.h on the host (tests/test_area_rule_cpu.py builds it with ASan +
// UBSan and compares what it writes with oracle/vo_gray.c).  The images live in heap blocks of their exact size, so a tap
// that reached past an image would be a sanitizer report.
//   area_check IN OUT   IN: int32 count, then per case int32 sh, sw, dh, dw and sh * sw bytes
//                       OUT: per case dh * dw bytes, formed with the taps in run form
// Where both ratios are below the eight-weight limit the case is formed a second time through AreaTaps tables, as the LDS
// kernels do; stdout gets one line "case <i> tables <same: 1|0, not applicable: -1>".
#include "vstab_area.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static void resize(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, bool tables)
{
    const AreaPlan pl = plan_area(sh, sw, dh, dw);
    const auto px = [=](int row, int col) { return (int)src[(size_t)row * sw + col]; };
    std::vector<AreaTaps> tx(tables ? dw : 0), ty(tables ? dh : 0);
    for (int x = 0; x < (int)tx.size(); x++) area_taps(x, sw, pl.scale_x, tx[x]);
    for (int y = 0; y < (int)ty.size(); y++) area_taps(y, sh, pl.scale_y, ty[y]);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int o;
            if (tables) {
                o = area_px(pl.mode, pl.isx, pl.isy, x, y, tx[x], ty[y], px);
            } else {
                AreaRun rx{}, ry{};
                if (pl.mode == AREA_GENERAL) { rx = area_run(x, sw, pl.scale_x); ry = area_run(y, sh, pl.scale_y); }
                o = area_px(pl.mode, pl.isx, pl.isy, x, y, rx, ry, px);
            }
            dst[(size_t)y * dw + x] = (uint8_t)o;
        }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (int i = 0; i < count; i++) {
        int32_t g[4];
        if (fread(g, 4, 4, in) != 4) return 2;
        const int sh = g[0], sw = g[1], dh = g[2], dw = g[3];
        if (sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || dh > sh || dw > sw) return 2;
        std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)sh * sw]), dst(new uint8_t[(size_t)dh * dw]), again(new uint8_t[(size_t)dh * dw]);
        if (fread(src.get(), 1, (size_t)sh * sw, in) != (size_t)sh * sw) return 2;
        resize(src.get(), sh, sw, dst.get(), dh, dw, false);
        if (fwrite(dst.get(), 1, (size_t)dh * dw, out) != (size_t)dh * dw) return 2;
        const AreaPlan pl = plan_area(sh, sw, dh, dw);
        int same = -1;
        if (pl.scale_x < AREA_TAPS_RATIO && pl.scale_y < AREA_TAPS_RATIO) {
            resize(src.get(), sh, sw, again.get(), dh, dw, true);
            same = memcmp(dst.get(), again.get(), (size_t)dh * dw) == 0 ? 1 : 0;
        }
        printf("case %d tables %d\n", i, same);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
