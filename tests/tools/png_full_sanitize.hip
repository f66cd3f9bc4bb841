// The host code of the two device PNG decoders (faster_rcnn_amd/csrc/png_dec_host.h, shared by png_dec.hip and png_dec_full.hip: the
// planner, the spans function and the validation half of the batch call parse untrusted bytes) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone program: no GPU, no Python, nothing preloaded.  Build and run from the repository root:
//
//   python -c "import sys; from tests import png_full_cases as F; [open('%s/%03d_%s.png' % (sys.argv[1], i, n), 'wb').write(d) for i, (n, d)
//              in enumerate(F.all_sound() + [(n, d) for n, d, _ in F.refusals()] + sorted(F.damaged().items()))]" CASES_DIR
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tests/tools/png_full_sanitize.hip faster_rcnn_amd/csrc/png_dec.hip faster_rcnn_amd/csrc/png_dec_full.hip \
//         -o png_full_sanitize
//   ./png_full_sanitize CASES_DIR/*.png
//
// For every file, through the entry points of revision 1 and through those of the full-format extension: the planner on the file and
// on every prefix of it (a file above 64 KiB: every prefix of its first and last 2048 bytes and every 257th between; the CRC of the
// whole chunks in front of a cut makes every prefix quadratic), each prefix with the bytes behind it poisoned so that a read past `len`
// is reported; the planner on the file with one byte changed (every byte in turn, XOR 0xFF and XOR 0x01; the same thinning for a large
// file), and what it still accepts through the spans function, the workspace size and the layout; the spans function on the file, on a
// plan of another file and with too little room; the batch call with null device pointers, and with pointers that are never followed
// and a table that the validation has to walk to its end before it refuses (an output one byte short, two items on the same output):
// it returns FRCNN_E_ARG before any launch or device call.  Exit status 0 and "clean" when the sanitizers reported nothing.
#include <sanitizer/asan_interface.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/frcnn_hip.h"
#include "../../include/ext/frcnn_hip_png_dec_full.h"

namespace frcnn {
static char g_message[512];
void set_error(const char* fmt, ...) {          // (the library's lives in boxes.hip)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
}
}  // namespace frcnn

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // (the HIP runtime's start-up allocations are not ours)

static int g_failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_failures; } } while (0)

// The two sets of entry points under one set of names.
struct Rev1 {
    using Plan = frcnn_png_dec_plan_t;
    using Item = frcnn_png_dec_batch_item_t;
    static constexpr const char* NAME = "revision 1";
    static int plan(const uint8_t* d, size_t n, Plan* p) { return frcnn_png_dec_plan(d, n, p); }
    static int spans(const uint8_t* d, size_t n, const Plan* p, uint32_t* s, size_t c) { return frcnn_png_dec_spans(d, n, p, s, c); }
    static size_t workspace(const Plan* p) { return frcnn_png_dec_workspace_bytes(p); }
    static size_t layout(const Plan* p, int n, uint64_t* w) { return frcnn_png_dec_batch_layout(p, n, w); }
    static size_t palette_bytes(const Plan&) { return 0; }
    static Item item(const Plan& p, uint64_t f, uint64_t o, uint64_t w) { return {p, f, o, w}; }
    template <class... A> static int decode(A... a) { return frcnn_png_decode_batch_u8(a...); }
};

struct Full {
    using Plan = frcnn_png_dec_full_plan_t;
    using Item = frcnn_png_dec_full_batch_item_t;
    static constexpr const char* NAME = "full format";
    static int plan(const uint8_t* d, size_t n, Plan* p) { return frcnn_png_dec_full_plan(d, n, p); }
    static int spans(const uint8_t* d, size_t n, const Plan* p, uint32_t* s, size_t c) { return frcnn_png_dec_full_spans(d, n, p, s, c); }
    static size_t workspace(const Plan* p) { return frcnn_png_dec_full_workspace_bytes(p); }
    static size_t layout(const Plan* p, int n, uint64_t* w) { return frcnn_png_dec_full_batch_layout(p, n, w); }
    static size_t palette_bytes(const Plan& p) { return p.colour_type == 3 ? FRCNN_PNG_DEC_FULL_PLTE_BYTES : 0; }
    static Item item(const Plan& p, uint64_t f, uint64_t o, uint64_t w) { return {p, f, o, w, f + p.stream_len}; }
    template <class... A> static int decode(A... a) { return frcnn_png_decode_full_batch_u8(a...); }
};

template <class D>
static void batch_validation(const std::vector<typename D::Plan>& plans) {
    const int n = (int)plans.size();
    std::vector<typename D::Item> items(n);
    std::vector<uint64_t> ws(n);
    const size_t ws_total = D::layout(plans.data(), n, ws.data());
    EXPECT(ws_total > 0, "%s: layout of %d plans", D::NAME, n);
    size_t files = 0, out = 0;
    for (int i = 0; i < n; ++i) {
        items[i] = D::item(plans[i], files, out, ws[i]);
        files += plans[i].stream_len + D::palette_bytes(plans[i]);
        out += (size_t)plans[i].h * plans[i].w * 3;
    }
    uint8_t* fake = reinterpret_cast<uint8_t*>(0x100000);                    // never followed
    const auto* dev = reinterpret_cast<const typename D::Item*>(0x200000);
    int32_t* status = reinterpret_cast<int32_t*>(0x300000);
    void* wsp = reinterpret_cast<void*>(0x400000);
    const typename D::Item* none = nullptr;
    uint8_t* null8 = nullptr;
    EXPECT(D::decode(items.data(), none, n, null8, files, 0, null8, out, (int32_t*)nullptr, (void*)nullptr, ws_total, (void*)nullptr) == FRCNN_E_ARG, "null pointers");
    EXPECT(D::decode(items.data(), dev, n, fake, files, 0, fake, out - 1, status, wsp, ws_total, (void*)nullptr) == FRCNN_E_ARG, "output short");
    EXPECT(D::decode(items.data(), dev, n, fake, files - 1, 0, fake, out, status, wsp, ws_total, (void*)nullptr) == FRCNN_E_ARG, "files short");
    EXPECT(D::decode(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total - 1, (void*)nullptr) == FRCNN_E_ARG, "workspace short");
    if (n >= 2) {
        items[n - 1].out_off = items[0].out_off;
        EXPECT(D::decode(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total, (void*)nullptr) == FRCNN_E_ARG, "same output");
        items[n - 1].out_off = out - (size_t)plans[n - 1].h * plans[n - 1].w * 3;
        items[n - 1].ws_off = items[0].ws_off;
        EXPECT(D::decode(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total, (void*)nullptr) == FRCNN_E_ARG, "same region");
    }
}

struct Counts { long prefixes = 0, corrupted = 0, accepted = 0, refused = 0; };

// What the planner accepted of ``n`` bytes at ``buf``, through the host functions that take a plan.
template <class D>
static void follow(const char* name, const uint8_t* buf, size_t n, const typename D::Plan& plan) {
    std::vector<uint32_t> spans(2 * (size_t)plan.idat_count);
    EXPECT(D::spans(buf, n, &plan, spans.data(), plan.idat_count) == FRCNN_OK, "%s: %s: spans", D::NAME, name);
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < plan.idat_count; ++k) {
        EXPECT((size_t)spans[2 * k] + spans[2 * k + 1] <= n, "%s: %s: span %u leaves the file", D::NAME, name, k);
        sum += spans[2 * k + 1];
    }
    EXPECT(sum == plan.stream_len, "%s: %s: spans sum", D::NAME, name);
    EXPECT(D::workspace(&plan) >= plan.inflated_len, "%s: %s: workspace", D::NAME, name);
    uint64_t at = 7;
    EXPECT(D::layout(&plan, 1, &at) == D::workspace(&plan) && at == 0, "%s: %s: layout", D::NAME, name);
}

template <class D>
static void one_file(const char* name, uint8_t* buf, size_t n, std::vector<typename D::Plan>& sound, typename D::Plan& other, Counts& c) {
    typename D::Plan plan = {}, cut = {};
    const int code = D::plan(buf, n, &plan);
    EXPECT(code == FRCNN_OK || code == FRCNN_E_UNSUPPORTED, "%s: %s: plan returned %d", D::NAME, name, code);
    const auto thinned = [n](size_t at) { return n > 65536 && at > 2048 && at + 2048 < n && at % 257; };
    for (size_t len = 0; len < n; ++len) {
        if (thinned(len)) continue;
        ASAN_POISON_MEMORY_REGION(buf + len, n - len);
        const int r = D::plan(buf, len, &cut);
        ASAN_UNPOISON_MEMORY_REGION(buf + len, n - len);
        EXPECT(r == FRCNN_E_UNSUPPORTED, "%s: %s: the prefix of %zu bytes returned %d", D::NAME, name, len, r);
        ++c.prefixes;
    }
    for (size_t at = 0; at < n; ++at) {
        if (thinned(at)) continue;
        for (const uint8_t flip : {(uint8_t)0xFF, (uint8_t)0x01}) {
            buf[at] ^= flip;
            const int r = D::plan(buf, n, &cut);
            EXPECT(r == FRCNN_OK || r == FRCNN_E_UNSUPPORTED, "%s: %s: byte %zu changed: plan returned %d", D::NAME, name, at, r);
            if (r == FRCNN_OK) follow<D>(name, buf, n, cut);
            buf[at] ^= flip;
            ++c.corrupted;
        }
    }
    if (code != FRCNN_OK) { ++c.refused; return; }
    ++c.accepted;
    follow<D>(name, buf, n, plan);
    std::vector<uint32_t> spans(2 * (size_t)plan.idat_count);
    EXPECT((size_t)plan.idat_off < n, "%s: %s: the first IDAT leaves the file", D::NAME, name);
    EXPECT(D::spans(buf, n, &plan, spans.data(), plan.idat_count - 1) == FRCNN_E_ARG, "%s: %s: spans without room", D::NAME, name);
    if (n > 1) {                                                            // a file that is not the plan's: a byte shorter, and another file's plan
        ASAN_POISON_MEMORY_REGION(buf + n - 1, 1);
        EXPECT(D::spans(buf, n - 1, &plan, spans.data(), plan.idat_count) == FRCNN_E_ARG, "%s: %s: spans of a cut file", D::NAME, name);
        ASAN_UNPOISON_MEMORY_REGION(buf + n - 1, 1);
    }
    if (other.file_len) {
        typename D::Plan mixed = other;
        mixed.file_len = (uint32_t)n;                                       // the walk then runs on offsets that are not this file's
        std::vector<uint32_t> room(2 * (size_t)mixed.idat_count + 2);
        (void)D::spans(buf, n, &mixed, room.data(), mixed.idat_count);
    }
    other = plan;
    sound.push_back(plan);
    if (sound.size() == FRCNN_PNG_DEC_BATCH_MAX) { batch_validation<D>(sound); sound.clear(); }
}

int main(int argc, char** argv) {
    std::vector<frcnn_png_dec_plan_t> sound1;
    std::vector<frcnn_png_dec_full_plan_t> sound;
    frcnn_png_dec_plan_t other1 = {};
    frcnn_png_dec_full_plan_t other = {};
    Counts rev1, full;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t n = (size_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (n && fread(buf, 1, n, f) != n) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        one_file<Rev1>(argv[a], buf, n, sound1, other1, rev1);
        one_file<Full>(argv[a], buf, n, sound, other, full);
        frcnn_png_dec_full_plan_t plan;
        if (frcnn_png_dec_full_plan(buf, n, &plan) == FRCNN_OK)
            EXPECT(plan.colour_type != 3 || (size_t)plan.plte_off + 3 * (size_t)plan.plte_entries <= n, "%s: the palette leaves the file", argv[a]);
        free(buf);
    }
    if (!sound1.empty()) batch_validation<Rev1>(sound1);
    if (!sound.empty()) batch_validation<Full>(sound);
    for (const auto& [name, c] : {std::pair<const char*, Counts>{Rev1::NAME, rev1}, {Full::NAME, full}})
        printf("%s: %d files (%ld accepted, %ld refused), %ld prefixes, %ld changed bytes\n", name, argc - 1, c.accepted, c.refused, c.prefixes, c.corrupted);
    printf("%s\n", g_failures ? "FAILED" : "clean");
    return g_failures ? 1 : 0;
}
