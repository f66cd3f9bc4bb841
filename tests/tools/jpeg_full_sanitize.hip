// The host code of the device decoder for progressive JPEG files (faster_rcnn_amd/csrc/jpeg_dec_full.hip: the planner parses untrusted
// bytes, the plan check is what the kernels' bounds rest on) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
// program: no GPU, no Python, nothing preloaded.  Build and run from the repository root:
//
//   python -c "import sys; from tests import jpeg_prog_cases as P; cases = sorted(P.files().items()) + sorted((n, d) for n, (d, _) in
//              P.unsupported().items()) + sorted(P.damaged().items()); [open('%s/%03d_%s.jpg' % (sys.argv[1], i, n), 'wb').write(d)
//              for i, (n, d) in enumerate(cases)]" CASES_DIR
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tests/tools/jpeg_full_sanitize.hip faster_rcnn_amd/csrc/jpeg_dec_full.hip -o jpeg_full_sanitize
//   ./jpeg_full_sanitize CASES_DIR/*.jpg
//
// For every file: frcnn_jpeg_dec_full_plan on the file and on every prefix of it (a file above 64 KiB: every prefix of its first and
// last 2048 bytes and every 257th between), each prefix with the bytes behind it poisoned so that a read past `len` is reported; the
// planner on the file with one byte of its HEADERS changed (every byte in front of the last scan's entropy-coded segment that lies
// outside the segments, in turn, XOR 0xFF and XOR 0x01; every 61st byte inside them); whatever it accepts goes through the plan check
// (the workspace size and the layout: both refuse what full_plan_fault refuses) and through the batch call with pointers that are never
// followed and an output one byte short: FRCNN_E_ARG before any launch or device call.  An accepted plan's offsets are checked against
// the file here as well.  Exit status 0 and "clean" when the sanitizers reported nothing.
#include <sanitizer/asan_interface.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/frcnn_hip.h"
#include "../../include/ext/frcnn_hip_jpeg_dec_full.h"

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

using Plan = frcnn_jpeg_dec_full_plan_t;
using Item = frcnn_jpeg_dec_full_batch_item_t;
struct Counts { long prefixes = 0, corrupted = 0, accepted = 0, refused = 0, followed = 0; };

// What the planner accepted of ``n`` bytes: every offset inside the file, the plan check agrees, the batch call refuses a short output.
static void follow(const char* name, size_t n, const Plan& plan, Counts& c) {
    ++c.followed;
    const size_t need = frcnn_jpeg_dec_full_workspace_bytes(&plan);
    EXPECT(need > 0 && need % 16 == 0, "%s: workspace of an accepted plan", name);
    uint64_t at = 7;
    EXPECT(frcnn_jpeg_dec_full_batch_layout(&plan, 1, &at) == need && at == 0, "%s: layout", name);
    EXPECT(plan.frame.file_len == n && plan.scans >= 1 && plan.scans <= FRCNN_JPEG_DEC_FULL_MAX_SCANS, "%s: file_len / scans", name);
    for (uint32_t i = 0; i < plan.scans && i < FRCNN_JPEG_DEC_FULL_MAX_SCANS; ++i) {
        const frcnn_jpeg_dec_full_scan_t& s = plan.scan[i];
        EXPECT((size_t)s.off + s.len <= n, "%s: scan %u leaves the file", name, i);
        for (int k = 0; k < 3; ++k) {
            EXPECT(!s.dc_off[k] || (size_t)s.dc_off[k] + 16 + s.dc_count[k] <= n, "%s: scan %u DC table %d leaves the file", name, i, k);
            EXPECT(!s.ac_off[k] || (size_t)s.ac_off[k] + 16 + s.ac_count[k] <= n, "%s: scan %u AC table %d leaves the file", name, i, k);
        }
    }
    for (int k = 0; k < plan.frame.components; ++k) EXPECT((size_t)plan.frame.dqt_off[k] + 64 <= n, "%s: DQT %d leaves the file", name, k);
    static Item item;
    item = Item{};
    item.plan = plan;
    const size_t out = (size_t)plan.frame.h * plan.frame.w * 3;
    uint8_t* fake = reinterpret_cast<uint8_t*>(0x100000);                    // never followed
    const Item* dev = reinterpret_cast<const Item*>(0x200000);
    int32_t* status = reinterpret_cast<int32_t*>(0x300000);
    void* wsp = reinterpret_cast<void*>(0x400000);
    EXPECT(frcnn_jpeg_decode_full_batch_u8(&item, dev, 1, fake, n, 0, fake, out - 1, status, wsp, need, nullptr) == FRCNN_E_ARG, "%s: output short", name);
    EXPECT(frcnn_jpeg_decode_full_batch_u8(&item, dev, 1, fake, n - 1, 0, fake, out, status, wsp, need, nullptr) == FRCNN_E_ARG, "%s: files short", name);
    EXPECT(frcnn_jpeg_decode_full_batch_u8(&item, dev, 1, fake, n, 0, fake, out, status, wsp, need - 1, nullptr) == FRCNN_E_ARG, "%s: workspace short", name);
    EXPECT(frcnn_jpeg_decode_full_u8(fake, &plan, dev, 0, fake, out - 1, status, wsp, need, nullptr) == FRCNN_E_ARG, "%s: single, output short", name);
    Plan bad = plan;                                                        // contradictions: refused by the plan check
    bad.frame.expected_blocks += 1;
    EXPECT(frcnn_jpeg_dec_full_workspace_bytes(&bad) == 0, "%s: block total off by one", name);
    bad = plan;
    bad.scan[plan.scans - 1].len = plan.frame.file_len;
    bad.scan[plan.scans - 1].off = 1;
    EXPECT(frcnn_jpeg_dec_full_workspace_bytes(&bad) == 0, "%s: a scan past the file", name);
}

static void one_file(const char* name, uint8_t* buf, size_t n, Counts& c) {
    static Plan plan, cut;
    const int code = frcnn_jpeg_dec_full_plan(buf, n, &plan);
    EXPECT(code == FRCNN_OK || code == FRCNN_E_UNSUPPORTED, "%s: plan returned %d", name, code);
    const auto thinned = [n](size_t at) { return n > 65536 && at > 2048 && at + 2048 < n && at % 257; };
    for (size_t len = 0; len < n; ++len) {
        if (thinned(len)) continue;
        ASAN_POISON_MEMORY_REGION(buf + len, n - len);
        const int r = frcnn_jpeg_dec_full_plan(buf, len, &cut);
        ASAN_UNPOISON_MEMORY_REGION(buf + len, n - len);
        EXPECT(r == FRCNN_E_UNSUPPORTED, "%s: the prefix of %zu bytes returned %d", name, len, r);
        ++c.prefixes;
    }
    // the headers: everything outside the entropy-coded segments (a refused file: all of it, thinned when it is large)
    std::vector<uint8_t> header(n, 1);
    if (code == FRCNN_OK)
        for (uint32_t i = 0; i < plan.scans; ++i)
            for (size_t at = plan.scan[i].off; at < (size_t)plan.scan[i].off + plan.scan[i].len && at < n; ++at) header[at] = 0;
    for (size_t at = 0; at < n; ++at) {
        if (header[at] ? thinned(at) : at % 61 != 0) continue;
        for (const uint8_t flip : {(uint8_t)0xFF, (uint8_t)0x01}) {
            buf[at] ^= flip;
            const int r = frcnn_jpeg_dec_full_plan(buf, n, &cut);
            EXPECT(r == FRCNN_OK || r == FRCNN_E_UNSUPPORTED, "%s: byte %zu changed: plan returned %d", name, at, r);
            if (r == FRCNN_OK) follow(name, n, cut, c);
            buf[at] ^= flip;
            ++c.corrupted;
        }
    }
    if (code != FRCNN_OK) { ++c.refused; return; }
    ++c.accepted;
    follow(name, n, plan, c);
}

int main(int argc, char** argv) {
    Counts c;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* buf = static_cast<uint8_t*>(malloc(size > 0 ? (size_t)size : 1));     // exactly the file: a read past it is a heap overflow
        if (size > 0 && fread(buf, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        one_file(argv[a], buf, (size_t)size, c);
        free(buf);
    }
    Plan none = {};
    EXPECT(frcnn_jpeg_dec_full_plan(nullptr, 4, &none) == FRCNN_E_ARG && frcnn_jpeg_dec_full_plan(nullptr, 0, &none) == FRCNN_E_UNSUPPORTED, "null file");
    EXPECT(frcnn_jpeg_dec_full_workspace_bytes(nullptr) == 0 && frcnn_jpeg_dec_full_workspace_bytes(&none) == 0, "null / empty plan");
    printf("%d files: %ld accepted, %ld refused; %ld prefixes, %ld single-byte changes (%ld of them still accepted and followed): %s\n", argc - 1,
           c.accepted, c.refused, c.prefixes, c.corrupted, c.followed - c.accepted, g_failures ? "FAILED" : "clean");
    return g_failures ? 1 : 0;
}
