// mlp_ln_probe.hip -- TEST ONLY (tests/test_mlp_ln_host.py): the library's own builder of the LayerNorm actor's operand image
// ("nig-mlp-ln-v1", csrc/nig_mlp_ln_stream.hpp) on the host.  Compiled host-only (hipcc --cuda-host-only), runs without a device and
// launches nothing.  Reads one case per line from stdin:
//   N <IN> <OUT> <weights file> <image file>
//       weights file: float32 W1 [IN][256], b1, g1, be1, W2 [256][256], b2, g2, be2, W3 [256][OUT], b3 back to back
//       image file:   the plan's floats put_ln_network wrote into a zeroed buffer
//       -> "<ok 0|1> <layer-1 chunks> <layer-1 tiles per chunk> <layer-1 records per tile> <chunks> <head chunk> <first float of the table> <floats>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "nig_mlp_ln_stream.hpp"

using namespace nig;

int main()
{
    char what;
    while (std::cin >> what) {
        int IN, OUT;
        std::string wfile, ifile;
        if (what != 'N' || !(std::cin >> IN >> OUT >> wfile >> ifile) || IN < 1 || OUT < 1) return 2;
        const size_t H = MLP_H;
        const size_t sizes[10] = {IN * H, H, H, H, H * H, H, H, H, H * (size_t)OUT, (size_t)OUT};
        size_t total = 0, off[10];
        for (int i = 0; i < 10; ++i) { off[i] = total; total += sizes[i]; }
        std::vector<float> w(total);
        FILE *f = fopen(wfile.c_str(), "rb");
        if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) return 3;
        fclose(f);
        const float *a[10];
        for (int i = 0; i < 10; ++i) a[i] = w.data() + off[i];
        const LnPlan p = ln_plan(IN);
        const size_t floats = p.floats();
        float *host = (float *)calloc(floats, sizeof(float));
        if (!host) return 4;
        const bool ok = put_ln_network(IN, OUT, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], host, floats);
        f = fopen(ifile.c_str(), "wb");
        if (!f || fwrite(host, sizeof(float), floats, f) != floats) return 5;
        fclose(f);
        free(host);
        std::cout << ok << ' ' << p.l1.chunks << ' ' << p.l1.tiles << ' ' << p.l1.records << ' ' << p.chunks << ' ' << p.head_chunk << ' '
                  << p.table() << ' ' << floats << '\n';
    }
    return 0;
}
