// Stand-alone host program for tests/test_preprocess_seg_host.py: the host side of mv_preprocess_u8_seg_fwd -- every record check,
// the tile and LDS sizing -- compiled for the host only (no device code, nothing launched) under AddressSanitizer and UBSan.
// The entry reaches for the device only after its host work, through device_status_word(); here that answers "not available",
// so a record set that passes every check and is sized ends with that one message, and a refused one with its own.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "preprocess.hip"

namespace mv {
static char g_err[1024];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
void set_kernel_name(const char*) {}
unsigned* device_status_word() { return nullptr; }
}  // namespace mv

namespace {

const char* const SIZED = "the device status word is not available";     // every check passed, the tile was chosen
int failures = 0;

struct Batch {
    std::vector<mv_preprocess_seg> rec;
    long long x_bytes = 0, m_bytes = 0;
    void add(int Hin, int Win, int Hr, int Wr, int top, int left, int flip) {
        rec.push_back({x_bytes, m_bytes, Hin, Win, Hr, Wr, top, left, flip, 0});
        x_bytes += 3LL * Hin * Win;
        m_bytes += 1LL * Hin * Win;
    }
};

void expect(const char* what, const Batch& b, int Hout, int Wout, int rc_want, const char* word, bool masks = true, int image_fill = 0,
            int mask_fill = 255, int in_chw = 0) {
    // exact-size heap copy: a read past the records is an ASan report
    std::vector<mv_preprocess_seg> rec(b.rec);
    char* base = (char*)0x10000000;
    const int rc = mv_preprocess_u8_seg_fwd(base, b.x_bytes, masks ? base + (1LL << 32) : nullptr, b.m_bytes, base + (2LL << 32),
                                            masks ? (int32_t*)(base + (3LL << 32)) : nullptr, rec.data(), (mv_preprocess_seg*)(base + (4LL << 32)),
                                            (const float*)(base + (5LL << 32)), (const float*)(base + (5LL << 32)) + 4, (int)rec.size(), Hout,
                                            Wout, image_fill, mask_fill, in_chw, MV_F32, 0, nullptr);
    const bool ok = rc == rc_want && strstr(mv::g_err, word) != nullptr;
    printf("%-34s rc %2d  %s%s\n", what, rc, mv::g_err, ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

}  // namespace

int main() {
    // the geometry sets of tests/_seg_augment_ref.py, crop 32 x 40
    const int sizes[6][2] = {{50, 37}, {37, 50}, {36, 36}, {20, 31}, {53, 47}, {400, 380}};
    const int flips[6] = {1, 0, 1, 1, 0, 1};
    const int sets[4][6][4] = {
        {{60, 44, 28, 4}, {37, 50, 3, 7}, {45, 45, 0, 0}, {40, 62, 5, 11}, {48, 43, 10, 2}, {36, 44, 2, 3}},
        {{24, 18, 0, 0}, {16, 22, 0, 0}, {20, 20, 0, 0}, {20, 31, 0, 0}, {31, 39, 0, 0}, {34, 33, 2, 0}},
        {{40, 30, 8, 0}, {24, 60, 0, 20}, {72, 72, 40, 32}, {40, 31, 3, 0}, {30, 47, 0, 7}, {40, 38, 8, 0}},
        {{5, 4, 0, 0}, {4, 5, 0, 0}, {4, 4, 0, 0}, {1, 3, 0, 0}, {5, 5, 0, 0}, {35, 34, 3, 0}}};
    const char* names[4] = {"inside", "pad", "mixed", "tiny"};
    for (int s = 0; s < 4; ++s) {
        Batch b;
        if (s == 3) b.add(9, 5, 1, 1, 0, 0, 1);
        for (int i = 0; i < 6; ++i) b.add(sizes[i][0], sizes[i][1], sets[s][i][0], sets[s][i][1], sets[s][i][2], sets[s][i][3], flips[i]);
        expect(names[s], b, 32, 40, MV_E_INVALID, SIZED);
        expect(names[s], b, 32, 40, MV_E_INVALID, SIZED, false, 114, 0, 1);
    }
    {   // the presets' shapes: 480 x 480 out of images around 500 x 375 resized to 260 .. 1040, and one image alone
        Batch b;
        b.add(500, 375, 1386, 1040, 906, 560, 0);
        b.add(375, 500, 260, 346, 0, 0, 1);
        b.add(333, 500, 520, 780, 40, 300, 1);
        expect("preset", b, 480, 480, MV_E_INVALID, SIZED);
        Batch one;
        one.add(1, 1, 1, 1, 0, 0, 0);
        expect("1 x 1", one, 1, 1, MV_E_INVALID, SIZED);
        expect("1 x 1 into 7 x 9", one, 7, 9, MV_E_INVALID, SIZED);
    }
    Batch good;
    good.add(40, 30, 50, 20, 18, 0, 0);
    good.add(400, 44, 36, 48, 4, 8, 1);
    expect("good", good, 32, 40, MV_E_INVALID, SIZED);
    Batch b = good;
    b.rec[1].offset += 1;
    expect("image past x", b, 32, 40, MV_E_INVALID, "image 1: 52800 bytes at offset 3601");
    b = good; b.rec[0].offset = -1;
    expect("negative offset", b, 32, 40, MV_E_INVALID, "image 0");
    b = good; b.rec[1].offset = INT64_MAX;
    expect("offset INT64_MAX", b, 32, 40, MV_E_INVALID, "image 1");
    b = good; b.rec[1].mask_offset = INT64_MAX;
    expect("mask offset INT64_MAX", b, 32, 40, MV_E_INVALID, "image 1: mask");
    expect("mask offset unused", b, 32, 40, MV_E_INVALID, SIZED, false);
    b = good; b.m_bytes -= 1;
    expect("mask past m", b, 32, 40, MV_E_INVALID, "image 1: mask of 17600 bytes");
    b = good; b.rec[0].Hin = 0;
    expect("Hin 0", b, 32, 40, MV_E_INVALID, "image 0: bad sizes");
    b = good; b.rec[1].Wr = -5;
    expect("Wr < 0", b, 32, 40, MV_E_INVALID, "image 1: bad sizes");
    b = good; b.rec[0].Hin = 46341; b.rec[0].Win = 46341;
    expect("image of 2^31 pixels", b, 32, 40, MV_E_INVALID, "image 0: 46341x46341 too large");
    b = good; b.rec[0].top = 19;
    expect("top past the last origin", b, 32, 40, MV_E_INVALID, "image 0: window 32x40 at (19, 0)");
    b = good; b.rec[0].top = INT32_MAX;
    expect("top INT32_MAX", b, 32, 40, MV_E_INVALID, "image 0: window");
    b = good; b.rec[0].left = 1;
    expect("left in a padded axis", b, 32, 40, MV_E_INVALID, "image 0: window");
    b = good; b.rec[1].left = -1;
    expect("left < 0", b, 32, 40, MV_E_INVALID, "image 1: window");
    b = good; b.rec[1].Hr = 33; b.rec[1].top = 1;
    expect("25 taps", b, 32, 40, MV_E_UNSUPPORTED, "image 1: 400x44 -> 33x48 needs up to 25 x 3 taps");
    b = good; b.rec[1].Hr = INT32_MAX; b.rec[1].Wr = INT32_MAX; b.rec[1].top = INT32_MAX - 32; b.rec[1].left = INT32_MAX - 40;
    expect("resized to INT32_MAX", b, 32, 40, MV_E_INVALID, SIZED);
    expect("image_fill 256", good, 32, 40, MV_E_INVALID, "image_fill 256", true, 256, 255);
    expect("mask_fill -1", good, 32, 40, MV_E_INVALID, "mask_fill -1", true, 0, -1);
    expect("Hout 0", good, 0, 40, MV_E_INVALID, "bad sizes");
    puts(failures ? "FAILED" : "all records answered as expected");
    return failures ? 1 : 0;
}
