// engine_lifecycle_main.cpp -- the life cycle of a tsnet_handle through the C ABI, as a program of its own for a sanitizer build of the HOST
// code: compiled with the six engine units and emu_runtime.cpp against tests/emu/include under -fsanitize=address,undefined (DESIGN.md gives
// the line).  The emulation header's hipMalloc is aligned_alloc, so LeakSanitizer sees every device buffer the engine does not release.
// Three lives on the tiny model (32 x 32 frames, n_downsampling 2, ngf 8: P = 64, C = 32; K = 2, max_batch 3):
//   create -> destroy;   create -> load, one NaN -> finalize refused -> destroy;
//   ... -> finalize refused -> reload -> finalize -> a forward of every kind, the training extras, stage_ptr, an uncollected timing -> destroy.
// Exit status 0 and no sanitizer report: every resource was released exactly once.  Not a pytest, and never for a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tsnet_abi.h"

namespace {

constexpr int K = 2, BMAX = 3, H = 32, W = 32, L = 2, P = 64, C = 32;
const char* kBad = "fuse_net.conv.weight";
float g_bad = std::nanf("");      // the non-finite value of the refused attempts; `inf` on the command line makes it an infinity

unsigned g_seed = 12345u;
float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / 16777216.0f - 0.5f; }

[[noreturn]] void die(const char* what, tsnet_handle h) {
    std::fprintf(stderr, "FAILED: %s (%s)\n", what, h ? tsnet_last_error(h) : "");
    std::exit(1);
}
void ok(int rc, const char* what, tsnet_handle h) { if (rc != TSNET_OK) die(what, h); }
void refused(int rc, const char* what, const char* text, tsnet_handle h) {
    if (rc == TSNET_OK || !std::strstr(tsnet_last_error(h), text)) die(what, h);
}

tsnet_handle create() {
    tsnet_cfg cfg{};
    cfg.label_nc = L; cfg.n_blocks = 1; cfg.n_downsampling = 2; cfg.n_source = K; cfg.ngf = 8; cfg.enc_blocks = 1; cfg.addcoords = 1;
    cfg.height = H; cfg.width = W; cfg.max_batch = BMAX;
    tsnet_handle h = nullptr;
    if (tsnet_create(&cfg, &h) != TSNET_OK) die("tsnet_create", nullptr);
    return h;
}

// every parameter, pseudo-random; `nan_in`: that one holds g_bad.  only: load that parameter alone
void load(tsnet_handle h, const char* nan_in, const char* only = nullptr) {
    for (int i = 0; i < tsnet_num_params(h); ++i) {
        const char* name = nullptr; int64_t shape[4]; int rank = 0;
        ok(tsnet_param_info(h, i, &name, shape, &rank), "tsnet_param_info", h);
        if (only && std::strcmp(name, only)) continue;
        size_t n = 1;
        for (int d = 0; d < rank; ++d) n *= (size_t)shape[d];
        std::vector<float> w(n);
        for (float& v : w) v = 0.5f * rnd();
        if (nan_in && !std::strcmp(name, nan_in)) w[n / 2] = g_bad;
        ok(tsnet_load_weights(h, name, w.data(), shape, rank), "tsnet_load_weights", h);
    }
}

struct Frames {         // B driving frames and K sources of batch B, wide form
    std::vector<float> img[K], lbl[K], bbox[K], tlbl, tbbox;
    const float *pi[K], *pl[K], *pb[K];
    explicit Frames(int B) {
        auto fill = [&](std::vector<float>& v, size_t n, int kind) {      // 0: image, 1: one-hot labels (channel 0), 2: a box mask
            v.assign(n, 0.f);
            for (size_t i = 0; i < n; ++i) v[i] = kind == 0 ? 200.f * rnd() : kind == 1 ? (float)(i % ((size_t)L * H * W) < (size_t)H * W) : (float)((i / W) % H >= 4 && (i / W) % H < 28);
        };
        for (int s = 0; s < K; ++s) {
            fill(img[s], (size_t)B * 3 * H * W, 0); fill(lbl[s], (size_t)B * L * H * W, 1); fill(bbox[s], (size_t)B * H * W, 2);
            pi[s] = img[s].data(); pl[s] = lbl[s].data(); pb[s] = bbox[s].data();
        }
        fill(tlbl, (size_t)B * L * H * W, 1); fill(tbbox, (size_t)B * H * W, 2);
    }
};

void full_life() {
    tsnet_handle h = create();
    load(h, kBad);
    refused(tsnet_finalize(h, nullptr), "finalize with a non-finite weight must be refused", "non-finite", h);
    load(h, nullptr, kBad);
    ok(tsnet_finalize(h, nullptr), "tsnet_finalize (retry)", h);
    std::vector<float> rgb((size_t)BMAX * 3 * H * W), flow((size_t)K * BMAX * P * 2);
    Frames f2(2), f1(1), f3(BMAX);
    const float* p = nullptr; size_t n = 0;
    // one-shot forward at B = 2, then the training extras on it
    ok(tsnet_forward(h, f2.pi, f2.pl, f2.pb, f2.tlbl.data(), f2.tbbox.data(), rgb.data(), flow.data(), 2, nullptr), "tsnet_forward", h);
    ok(tsnet_stage_ptr(h, "src_fea", &p, &n), "tsnet_stage_ptr", h);
    if (n != (size_t)K * 2 * P * C) die("src_fea count after a one-shot forward", h);
    std::vector<float> warp((size_t)K * 2 * 3 * H * W), losses(2);
    ok(tsnet_train_extras(h, f2.pi, f2.img[0].data(), 2, warp.data(), losses.data(), nullptr), "tsnet_train_extras", h);
    // the per-batch cache
    ok(tsnet_set_sources(h, f2.pi, f2.pl, f2.pb, 2, nullptr), "tsnet_set_sources", h);
    ok(tsnet_forward_target(h, f2.tlbl.data(), f2.tbbox.data(), rgb.data(), nullptr, 2, nullptr), "tsnet_forward_target", h);
    // a shared source set: the extras are refused
    ok(tsnet_set_sources_shared(h, f1.pi, f1.pl, f1.pb, nullptr), "tsnet_set_sources_shared", h);
    ok(tsnet_forward_target(h, f3.tlbl.data(), f3.tbbox.data(), rgb.data(), flow.data(), BMAX, nullptr), "tsnet_forward_target (shared)", h);
    ok(tsnet_stage_ptr(h, "src_fea", &p, &n), "tsnet_stage_ptr", h);
    if (n != (size_t)K * P * C) die("src_fea count after a forward on a shared source set", h);
    refused(tsnet_train_extras(h, f3.pi, f3.img[0].data(), BMAX, warp.data(), losses.data(), nullptr), "train_extras on a shared set", "shared source set", h);
    // the bank: the extras are refused
    ok(tsnet_bank_put(h, 1, K, f1.pi, f1.pl, f1.pb, nullptr, nullptr), "tsnet_bank_put", h);
    const int slots[K * BMAX] = {2, 2, 1, 1, 1, 2};
    ok(tsnet_forward_bank(h, slots, K, f3.tlbl.data(), f3.tbbox.data(), rgb.data(), flow.data(), BMAX, nullptr), "tsnet_forward_bank", h);
    ok(tsnet_stage_ptr(h, "src_fea", &p, &n), "tsnet_stage_ptr", h);
    if (n != (size_t)K * BMAX * P * C) die("src_fea count after a forward on the bank", h);
    refused(tsnet_train_extras(h, f3.pi, f3.img[0].data(), BMAX, warp.data(), losses.data(), nullptr), "train_extras on a bank", "source bank", h);
    // timing on for one forward, never read: the records go with the handle
    ok(tsnet_timing_enable(h, 1), "tsnet_timing_enable", h);
    ok(tsnet_forward(h, f2.pi, f2.pl, f2.pb, f2.tlbl.data(), f2.tbbox.data(), rgb.data(), nullptr, 2, nullptr), "tsnet_forward (timed)", h);
    for (float v : rgb) if (!std::isfinite(v)) die("a non-finite output", h);
    tsnet_destroy(h);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "inf")) g_bad = INFINITY;
    tsnet_destroy(create());
    {
        tsnet_handle h = create();
        load(h, kBad);
        refused(tsnet_finalize(h, nullptr), "finalize with a non-finite weight must be refused", "non-finite", h);
        tsnet_destroy(h);
    }
    full_life();
    std::puts("engine_lifecycle: ok");
    return 0;
}
