// The host code of the full-format PNG decoder (faster_rcnn_amd/csrc/png_dec_full.hip: the planner, the spans function and the
// validation half of the batch call parse untrusted bytes) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
// program: no GPU, no Python, nothing preloaded.  Build and run from the repository root:
//
//   python -c "import sys; from tests import png_full_cases as F; [open('%s/%03d_%s.png' % (sys.argv[1], i, n), 'wb').write(d) for i, (n, d)
//              in enumerate(F.all_sound() + [(n, d) for n, d, _ in F.refusals()] + sorted(F.damaged().items()))]" CASES_DIR
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tests/tools/png_full_sanitize.hip faster_rcnn_amd/csrc/png_dec_full.hip -o png_full_sanitize
//   ./png_full_sanitize CASES_DIR/*.png
//
// For every file: frcnn_png_dec_full_plan on the file and on every prefix of it (a file above 64 KiB: every prefix of its first and last
// 2048 bytes and every 257th between; the CRC of the whole chunks in front of a cut makes every prefix quadratic), each prefix with the
// bytes behind it poisoned so that a read past `len` is reported; frcnn_png_dec_full_spans on the file, on a plan of another file and
// with too little room; the batch call with null device pointers, and with pointers that are never followed and a table that the
// validation has to walk to its end before it refuses (an output one byte short, two items on the same output): it returns
// FRCNN_E_ARG before any launch or device call.  Exit status 0 and "clean" when the sanitizers reported nothing.
#include <sanitizer/asan_interface.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static void batch_validation(const std::vector<frcnn_png_dec_full_plan_t>& plans) {
    const int n = (int)plans.size();
    std::vector<frcnn_png_dec_full_batch_item_t> items(n);
    std::vector<uint64_t> ws(n);
    const size_t ws_total = frcnn_png_dec_full_batch_layout(plans.data(), n, ws.data());
    EXPECT(ws_total > 0, "layout of %d plans", n);
    size_t files = 0, out = 0;
    for (int i = 0; i < n; ++i) {
        items[i].plan = plans[i];
        items[i].file_off = files;
        items[i].plte_off = files + plans[i].stream_len;
        items[i].out_off = out;
        items[i].ws_off = ws[i];
        files += plans[i].stream_len + (plans[i].colour_type == 3 ? FRCNN_PNG_DEC_FULL_PLTE_BYTES : 0);
        out += (size_t)plans[i].h * plans[i].w * 3;
    }
    uint8_t* fake = reinterpret_cast<uint8_t*>(0x100000);                    // never followed
    const auto* dev = reinterpret_cast<const frcnn_png_dec_full_batch_item_t*>(0x200000);
    int32_t* status = reinterpret_cast<int32_t*>(0x300000);
    void* wsp = reinterpret_cast<void*>(0x400000);
    EXPECT(frcnn_png_decode_full_batch_u8(items.data(), nullptr, n, nullptr, files, 0, nullptr, out, nullptr, nullptr, ws_total, nullptr) == FRCNN_E_ARG, "null pointers");
    EXPECT(frcnn_png_decode_full_batch_u8(items.data(), dev, n, fake, files, 0, fake, out - 1, status, wsp, ws_total, nullptr) == FRCNN_E_ARG, "output short");
    EXPECT(frcnn_png_decode_full_batch_u8(items.data(), dev, n, fake, files - 1, 0, fake, out, status, wsp, ws_total, nullptr) == FRCNN_E_ARG, "files short");
    EXPECT(frcnn_png_decode_full_batch_u8(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total - 1, nullptr) == FRCNN_E_ARG, "workspace short");
    if (n >= 2) {
        items[n - 1].out_off = items[0].out_off;
        EXPECT(frcnn_png_decode_full_batch_u8(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total, nullptr) == FRCNN_E_ARG, "same output");
        items[n - 1].out_off = out - (size_t)plans[n - 1].h * plans[n - 1].w * 3;
        items[n - 1].ws_off = items[0].ws_off;
        EXPECT(frcnn_png_decode_full_batch_u8(items.data(), dev, n, fake, files, 0, fake, out, status, wsp, ws_total, nullptr) == FRCNN_E_ARG, "same region");
    }
}

int main(int argc, char** argv) {
    std::vector<frcnn_png_dec_full_plan_t> sound;
    frcnn_png_dec_full_plan_t other = {};
    long prefixes = 0, accepted = 0, refused = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t n = (size_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* buf = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (n && fread(buf, 1, n, f) != n) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        frcnn_png_dec_full_plan_t plan = {}, cut = {};
        const int code = frcnn_png_dec_full_plan(buf, n, &plan);
        EXPECT(code == FRCNN_OK || code == FRCNN_E_UNSUPPORTED, "%s: plan returned %d", argv[a], code);
        for (size_t len = 0; len < n; ++len) {
            if (n > 65536 && len > 2048 && len + 2048 < n && len % 257) continue;
            ASAN_POISON_MEMORY_REGION(buf + len, n - len);
            const int c = frcnn_png_dec_full_plan(buf, len, &cut);
            ASAN_UNPOISON_MEMORY_REGION(buf + len, n - len);
            EXPECT(c == FRCNN_E_UNSUPPORTED, "%s: the prefix of %zu bytes returned %d", argv[a], len, c);
            ++prefixes;
        }
        if (code == FRCNN_OK) {
            ++accepted;
            std::vector<uint32_t> spans(2 * (size_t)plan.idat_count);
            EXPECT(frcnn_png_dec_full_spans(buf, n, &plan, spans.data(), plan.idat_count) == FRCNN_OK, "%s: spans", argv[a]);
            unsigned long long sum = 0;
            for (uint32_t k = 0; k < plan.idat_count; ++k) {
                EXPECT((size_t)spans[2 * k] + spans[2 * k + 1] <= n, "%s: span %u leaves the file", argv[a], k);
                sum += spans[2 * k + 1];
            }
            EXPECT(sum == plan.stream_len, "%s: spans sum", argv[a]);
            EXPECT(plan.colour_type != 3 || (size_t)plan.plte_off + 3 * (size_t)plan.plte_entries <= n, "%s: the palette leaves the file", argv[a]);
            EXPECT(frcnn_png_dec_full_spans(buf, n, &plan, spans.data(), plan.idat_count - 1) == FRCNN_E_ARG, "%s: spans without room", argv[a]);
            if (n > 1) {                                                        // a file that is not the plan's: a byte shorter, and another file's plan
                ASAN_POISON_MEMORY_REGION(buf + n - 1, 1);
                EXPECT(frcnn_png_dec_full_spans(buf, n - 1, &plan, spans.data(), plan.idat_count) == FRCNN_E_ARG, "%s: spans of a cut file", argv[a]);
                ASAN_UNPOISON_MEMORY_REGION(buf + n - 1, 1);
            }
            if (other.file_len) {
                frcnn_png_dec_full_plan_t mixed = other;
                mixed.file_len = (uint32_t)n;                                   // the walk then runs on offsets that are not this file's
                std::vector<uint32_t> room(2 * (size_t)mixed.idat_count + 2);
                (void)frcnn_png_dec_full_spans(buf, n, &mixed, room.data(), mixed.idat_count);
            }
            EXPECT(frcnn_png_dec_full_workspace_bytes(&plan) >= plan.inflated_len, "%s: workspace", argv[a]);
            other = plan;
            sound.push_back(plan);
            if (sound.size() == FRCNN_PNG_DEC_BATCH_MAX) { batch_validation(sound); sound.clear(); }
        } else {
            ++refused;
        }
        free(buf);
    }
    if (!sound.empty()) batch_validation(sound);
    printf("%d files (%ld accepted, %ld refused), %ld prefixes: %s\n", argc - 1, accepted, refused, prefixes, g_failures ? "FAILED" : "clean");
    return g_failures ? 1 : 0;
}
