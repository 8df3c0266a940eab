// mlp_shape_probe.hip -- TEST ONLY (tests/test_mlp_shape_host.py): the library's own builder of the shaped actor's operand image
// ("nig-mlp-shape-v1") on the host.  Compiled host-only (hipcc --cuda-host-only), runs without a device and launches nothing.
// Reads one case per line from stdin:
//   C <S> <nh> <d0> <d1> <d2>
//       -> "<kind>": shape_class_of (0 none, 1 reference, 2 128x128, 3 512x256, 4 512x512, 5 256x256x256)
//   N <kind> <IN> <OUT> <nh> <d0> <d1> <d2> <weights file> <image file>
//       weights file: float32 W[0], b[0], W[1], b[1], .. back to back, W[l] [in_l][out_l] row-major, unpadded
//       image file:   the plan's floats put_shape_network wrote into a zeroed buffer (kind 1: put_reference_padded's MLP_STREAM_FLOATS)
//       -> "<ok 0|1> <chrec> <l1_rec> <l1_tiles> <l1_chunks> <kch of layer 2> <kch of layer 3> <chunks> <floats>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "nig_mlp_shape_stream.hpp"

using namespace nig;

int main()
{
    char what;
    while (std::cin >> what) {
        if (what == 'C') {
            int S, nh, d[3];
            if (!(std::cin >> S >> nh >> d[0] >> d[1] >> d[2])) return 2;
            std::cout << (nh >= 1 && nh <= 3 ? shape_class_of(nh, d, S) : SHAPE_KIND_NONE) << '\n';
            continue;
        }
        int kind, IN, OUT, nh, d[3];
        std::string wfile, ifile;
        if (what != 'N' || !(std::cin >> kind >> IN >> OUT >> nh >> d[0] >> d[1] >> d[2] >> wfile >> ifile)) return 2;
        if (kind < SHAPE_KIND_REFERENCE || kind > SHAPE_KIND_3 || nh < 2 || nh > 3) return 2;
        size_t total = 0;
        std::vector<size_t> wo(nh + 1), bo(nh + 1);
        for (int l = 0, in = IN; l <= nh; ++l) {
            const int out = l < nh ? d[l] : OUT;
            wo[l] = total; total += (size_t)in * out;
            bo[l] = total; total += out;
            in = out;
        }
        std::vector<float> w(total);
        FILE *f = fopen(wfile.c_str(), "rb");
        if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) return 3;
        fclose(f);
        const float *W[4], *b[4];
        for (int l = 0; l <= nh; ++l) { W[l] = w.data() + wo[l]; b[l] = w.data() + bo[l]; }
        const ShapePlan p = shape_plan(SHAPE_CLASSES[kind], IN);
        const size_t floats = kind == SHAPE_KIND_REFERENCE ? (size_t)MLP_STREAM_FLOATS : p.floats();
        float *host = (float *)calloc(floats, sizeof(float));
        if (!host) return 4;
        bool ok;
        if (kind == SHAPE_KIND_REFERENCE) {
            std::vector<float> pad(reference_pad_floats(IN, OUT), 0.0f);
            ok = put_reference_padded(IN, OUT, d, W, b, pad.data(), host, floats);
        } else {
            ok = put_shape_network(SHAPE_CLASSES[kind], IN, OUT, nh, d, W, b, host, floats);
        }
        f = fopen(ifile.c_str(), "wb");
        if (!f || fwrite(host, sizeof(float), floats, f) != floats) return 5;
        fclose(f);
        free(host);
        std::cout << ok << ' ' << p.chrec << ' ' << p.l1_rec << ' ' << p.l1_tiles << ' ' << p.l1_chunks << ' ' << p.kch[1] << ' ' << p.kch[2] << ' '
                  << p.chunks << ' ' << floats << '\n';
    }
    return 0;
}
