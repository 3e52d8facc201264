// Stand-alone replay of the routing rule (eqxvision_amd/csrc/route.h): host compiler only, no HIP, nothing launched.
// stdin: one recorded call per line -- "<entry> <nargs> <args...> <scratch bytes> <nflags> (<flag> <value>)..." (pointer
// arguments as 0 / 1 = NULL / set; tests/test_route_host.py writes the lines from tests/data/routes.json).
// stdout: per line "<kernel name or -> <Kern as int> <tile>".
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../eqxvision_amd/csrc/route.h"

using namespace mv;

static std::map<std::string, int> g_flags;
static int flag(const char* name) {
    auto it = g_flags.find(name);
    return it == g_flags.end() ? 0 : it->second;
}

// did the igemm8 launch of this route take the scratch on offer?  (igemm8.hip: igemm8_go)
static bool took_scratch(Route r, long long M, int K, long long nk, long long scratch) {
    if (r.kern != Kern::igemm8 || r.tile < 2) return false;
    const int bm = r.tile == 2 ? 128 : 256, bn = r.tile == 3 ? 128 : 256;
    const size_t need = splitk_need_bytes(((M + bm - 1) / bm) * ((K + bn - 1) / bn), nk, flag);
    return need && (size_t)scratch >= need;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string entry;
        size_t nargs = 0, nflags = 0;
        long long scratch = 0;
        in >> entry >> nargs;
        std::vector<long long> a(nargs);
        for (auto& v : a) in >> v;
        in >> scratch >> nflags;
        g_flags.clear();
        for (size_t i = 0; i < nflags; ++i) {
            std::string k;
            int v;
            in >> k >> v;
            g_flags[k] = v;
        }
        if (!in) {
            std::cerr << "bad line: " << line << "\n";
            return 2;
        }
        Route r = {Kern::generic, 0};
        const char* name = "";
        if (entry == "mv_conv2d_nhwc_fwd" && nargs == 23) {        // x w scale shift residual y | N H W C K R S sh sw ph pw dh dw groups act in out
            const long long* d = &a[6];
            const ConvShape s = {(int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], (int)d[6], (int)d[7], (int)d[8],
                                 (int)d[9], (int)d[10], (int)d[11], (int)d[12], (int)d[13], (int)d[14], (int)d[15], (int)d[16],
                                 a[4] != 0, a[2] != 0};
            r = route_conv(s, flag);
            name = kernel_name(r, s.dense(), s, false, took_scratch(r, s.M(), s.K, (long long)s.R * s.S * (s.C / 64), scratch), flag);
        } else if (entry == "mv_linear_fwd" && nargs == 12) {      // x w scale shift residual y | M N K act in out
            const ConvShape s = linear_shape(a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10], (int)a[11], a[4] != 0, a[2] != 0);
            r = route_linear(s, flag);
            name = kernel_name(r, true, s, false, took_scratch(r, s.M(), s.K, s.C / 64, scratch), flag);
        } else if (entry == "mv_linear_heads_fwd" && nargs == 11) {        // x w scale shift y | M N K tokens dh dtype
            const ConvShape s = linear_shape(a[5], (int)a[6], (int)a[7], MV_ACT_NONE, MV_BF16, MV_BF16, false, a[2] != 0);
            r = route_linear_heads(a[5], (int)a[6], (int)a[7], flag);
            name = kernel_name(r, true, s, false, took_scratch(r, s.M(), s.K, s.C / 64, scratch), flag);
        } else if (entry == "mv_conv1x1_dual_fwd" && nargs == 17) {        // x x2 w scale shift y | N Ho Wo C1 H2 W2 C2 stride2 K act dtype
            const long long M = a[6] * a[7] * a[8];
            const int C1 = (int)a[9], C2 = (int)a[12], K = (int)a[14];
            const ConvShape s = linear_shape(M, K, C1, (int)a[15], MV_BF16, MV_BF16, false, a[3] != 0);
            r = route_conv1x1_dual(M, C1, C2, K, (int)a[13], (int)a[16], flag);
            name = kernel_name(r, true, s, true, took_scratch(r, M, K, (C1 + C2) / 64, scratch), flag);
        } else if (entry == "mv_linear_split_fwd" && nargs == 12) {        // x w_hi_lo scale shift residual y | M N K act in out
            const ConvShape s = linear_shape(a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10], (int)a[11], a[4] != 0, a[2] != 0);
            r = route_linear_split(a[6], (int)a[7], (int)a[8], flag);
            name = kernel_name(r, true, s, true, took_scratch(r, s.M(), s.K, 2 * (s.C / 64), scratch), flag);
        } else if (entry == "mv_conv2d_nhwc_grouped64_fwd") {
            r = {Kern::igemm128, 64};                               // its own entry: one kernel, no rule
            name = kGrouped64Name;
        } else {
            std::cerr << "unknown entry: " << line << "\n";
            return 2;
        }
        std::cout << (*name ? name : "-") << " " << (int)r.kern << " " << r.tile << "\n";
    }
    return 0;
}
