// Host evaluation of sceneego_amd/csrc/conv3d_pack.h (the packed-weight format of the float32 3D convolutions): every element of
// every section and of the bias, by the functions the pack kernels of conv3d_pack.hip call.  Built with g++ and run by
// tests/test_conv_pack_host.py, which writes the layers and compares the buffers with tests/conv_pack_model.py.
//   usage: conv3d_pack_check IN OUT [IN OUT ...]
//   IN : int32 cout, cin, cin_pad, ksize, transposed, has_bn, has_bias; float32 eps; float32 w[cout * cin * taps],
//        then b[cout] (has_bias), gamma, beta, mean, var [cout] (has_bn)
//   OUT: int64 total; float32 wpack[total]; float32 bpack[round_up16(cout)]     (both start out as NaN)
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../sceneego_amd/csrc/conv3d_pack.h"

static bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
    v.resize(n);
    return fread(v.data(), sizeof(float), n, f) == n;
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) return 2;
    int hdr[7];
    float eps;
    std::vector<float> w, b, gamma, beta, mean, var;
    bool ok = fread(hdr, sizeof(int), 7, f) == 7 && fread(&eps, sizeof(float), 1, f) == 1;
    const int cout = hdr[0], cin = hdr[1], cin_pad = hdr[2], ksize = hdr[3], transposed = hdr[4];
    ok = ok && cout > 0 && cin > 0 && cin_pad >= cin && cin_pad % 16 == 0 && (transposed ? ksize == 2 : (ksize == 1 || ksize == 3 || ksize == 7));
    if (ok) {
        const size_t taps = transposed ? 8 : (size_t)ksize * ksize * ksize;
        ok = read_floats(f, w, (size_t)cout * cin * taps);
        if (ok && hdr[6]) ok = read_floats(f, b, cout);
        if (ok && hdr[5]) ok = read_floats(f, gamma, cout) && read_floats(f, beta, cout) && read_floats(f, mean, cout) && read_floats(f, var, cout);
    }
    fclose(f);
    if (!ok) return 3;

    const SePackSource src = {w.data(), hdr[5] ? gamma.data() : nullptr, hdr[5] ? var.data() : nullptr, eps, cout, cin, cin_pad, ksize, transposed};
    const SePackLayout l = se_conv3d_pack_layout(cout, cin_pad, ksize, transposed);
    std::vector<float> wpack((size_t)l.total, NAN), bpack((size_t)round_up16(cout), NAN);
    for (int sec = 0; sec < SE_PACK_SECTIONS; ++sec)
        for (long long t = 0; t < l.elems[sec]; ++t) wpack[(size_t)(l.at[sec] + t)] = se_pack_value(sec, src, t);
    for (int t = 0; t < round_up16(cout); ++t)
        bpack[t] = se_pack_bias(src, hdr[6] ? b.data() : nullptr, hdr[5] ? beta.data() : nullptr, hdr[5] ? mean.data() : nullptr, t);

    FILE* o = fopen(out_path, "wb");
    if (!o) return 4;
    const long long total = l.total;
    ok = fwrite(&total, sizeof(total), 1, o) == 1 && fwrite(wpack.data(), sizeof(float), wpack.size(), o) == wpack.size() &&
         fwrite(bpack.data(), sizeof(float), bpack.size(), o) == bpack.size();
    return fclose(o) == 0 && ok ? 0 : 5;
}

int main(int argc, char** argv) {
    if (argc < 3 || (argc & 1) == 0) {
        fprintf(stderr, "usage: %s IN OUT [IN OUT ...]\n", argv[0]);
        return 1;
    }
    for (int i = 1; i + 1 < argc; i += 2) {
        const int rc = run(argv[i], argv[i + 1]);
        if (rc) {
            fprintf(stderr, "%s: failed (%d)\n", argv[i], rc);
            return rc;
        }
    }
    return 0;
}
