// mlp_stream_probe.hip -- TEST ONLY (tests/test_mlp_stream.py): the library's own operand-stream builder on the host.  Compiled
// host-only (hipcc --cuda-host-only), runs without a device and launches nothing.  Reads one case per line from stdin:
//   K
//       -> "<MLP_CHREC> <MLP_PER> <MLP_STREAM_FLOATS> <MLP_CSTREAM_FLOATS>"
//   N <IN> <OUT> <floats> <weights file> <image file>
//       weights file: float32 W1[IN][256], b1[256], W2[256][256], b2[256], W3[256][OUT], b3[OUT], back to back
//       image file:   the <floats> floats put_network wrote into a zeroed buffer
//       -> "<ok 0|1> <padded width> <records per tile> <layer-1 chunks> <tiles per chunk> <pieces per layer-1 chunk>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "nig_mlp_stream.hpp"

using namespace nig;

int main()
{
    char what;
    while (std::cin >> what) {
        if (what == 'K') {
            std::cout << MLP_CHREC << ' ' << MLP_PER << ' ' << MLP_STREAM_FLOATS << ' ' << MLP_CSTREAM_FLOATS << '\n';
            continue;
        }
        int IN, OUT;
        size_t floats;
        std::string wfile, ifile;
        if (what != 'N' || !(std::cin >> IN >> OUT >> floats >> wfile >> ifile)) return 2;
        const int H = MLP_H;
        std::vector<float> w((size_t)IN * H + H + (size_t)H * H + H + (size_t)H * OUT + OUT);
        FILE *f = fopen(wfile.c_str(), "rb");
        if (!f || fread(w.data(), sizeof(float), w.size(), f) != w.size()) return 3;
        fclose(f);
        const float *W1 = w.data(), *b1 = W1 + (size_t)IN * H, *W2 = b1 + H, *b2 = W2 + (size_t)H * H, *W3 = b2 + H, *b3 = W3 + (size_t)H * OUT;
        float *host = (float *)calloc(floats, sizeof(float));
        if (!host) return 4;
        const bool ok = put_network(IN, OUT, W1, b1, W2, b2, W3, b3, host, floats);
        f = fopen(ifile.c_str(), "wb");
        if (!f || fwrite(host, sizeof(float), floats, f) != floats) return 5;
        fclose(f);
        free(host);
        const MlpLayer1 L = mlp_layer1(IN);
        std::cout << ok << ' ' << L.width << ' ' << L.records << ' ' << L.chunks << ' ' << L.tiles << ' ' << L.pieces << '\n';
    }
    return 0;
}
