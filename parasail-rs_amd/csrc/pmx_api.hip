// pmx_api.hip -- the C ABI of libparasail_amd.so (declared in include/parasail_amd.h).
//
// Host side of the drop-in boundary: the `parasail_*` symbols parasail-rs binds through
// libparasail-sys (/root/reference/src/aligner/mod.rs:4-7, src/alignment/mod.rs:6-23,
// src/matrix/mod.rs:7-11, src/profile/mod.rs:5-32) plus the additive `pmx_*` batch entries.
// All DP arithmetic is done by the HIP kernels (pmx_sw16.hip, pmx_general.hip); this file
// owns handles, dispatch-name parsing, device staging and result marshalling only.
#include "pmx_common.h"
#include "pmx_switches.h"
#include "pmx_strip.h"
#include <chrono>
#include <future>
#include "pmx_matrices.h"

#include <cctype>
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

// ---- the switch table (pmx_switches.h) ------------------------------------------------------------------------------
static const PmxSwitchDoc g_switches[] = {
#define X(name, kind, what) {name, kind, what},
    PMX_SWITCH_TABLE(X)
#undef X
};
const char *pmx_env(const char *name)
{
    for (const PmxSwitchDoc &d : g_switches)
        if (!strcmp(d.name, name)) return getenv(name);
    fprintf(stderr, "libparasail_amd: environment switch %s is not in pmx_switches.h\n", name);
    abort();
}
// "NAME\tkind\twhat\n" per switch (static storage)
extern "C" const char *pmx_switches(void)
{
    static const std::string text = []() {
        std::string t;
        for (const PmxSwitchDoc &d : g_switches) { t += d.name; t += '\t'; t += d.kind; t += '\t'; t += d.what; t += '\n'; }
        return t;
    }();
    return text.c_str();
}

// ============================================================================ errors ====
static thread_local char g_err[512] = "";
static void set_err(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
extern "C" const char *pmx_last_error(void) { return g_err; }
extern "C" const char *pmx_version(void) { return "parasail_amd 0.1.0 (gfx950)"; }

// The product path has no CPU fallback: a failing HIP call in a function whose signature
// cannot report errors (the reference never checks alignment results for NULL,
// src/aligner/mod.rs:411-429) is fatal and loud.
[[noreturn]] static void die(const char *what, hipError_t e)
{
    fprintf(stderr, "libparasail_amd: fatal: %s: %s (no CPU fallback exists)\n", what,
            e == hipSuccess ? "" : hipGetErrorString(e));
    abort();
}
#define HIP_OR_DIE(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) die(#expr, e__); } while (0)
#define HIP_OR_RET(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { \
    set_err("%s: %s", #expr, hipGetErrorString(e__)); return -(int)e__; } } while (0)

extern "C" int pmx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int pmx_set_device(int device)
{
    HIP_OR_RET(hipSetDevice(device));
    return 0;
}

// =========================================================================== matrices ===
struct MatrixBox {               // owns everything a non-builtin parasail_matrix_t points to
    parasail_matrix_t m;
    std::vector<int> scores, mapper;
    std::string name, alphabet, query;
};

static void finish_box(MatrixBox *b, int type, int length, int size, bool user)
{
    b->m.name = b->name.c_str();
    b->m.matrix = b->scores.data();
    b->m.mapper = b->mapper.data();
    b->m.size = size;
    int mx = INT32_MIN, mn = INT32_MAX;
    for (int v : b->scores) { mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
    b->m.max = mx; b->m.min = mn;
    b->m.user_matrix = user ? b->scores.data() : nullptr;
    b->m.type = type;
    b->m.length = length;
    b->m.alphabet = b->alphabet.c_str();
    b->m.query = b->query.empty() ? nullptr : b->query.c_str();
}

static std::mutex g_mx_mutex;
static std::unordered_map<const parasail_matrix_t *, MatrixBox *> g_boxes;   // live non-builtin matrices

static parasail_matrix_t *publish(MatrixBox *b)
{
    std::lock_guard<std::mutex> lk(g_mx_mutex);
    g_boxes[&b->m] = b;
    return &b->m;
}

static void fill_mapper(std::vector<int> &mapper, const std::string &alphabet, int wildcard)
{
    mapper.assign(256, wildcard);
    for (size_t i = 0; i < alphabet.size(); ++i) {
        const unsigned char c = (unsigned char)alphabet[i];
        mapper[(unsigned char)toupper(c)] = (int)i;
        mapper[(unsigned char)tolower(c)] = (int)i;
    }
}

// src/matrix/mod.rs:34-44.  size = alphabet + 1 wildcard row/col (bound size-2 at :228-236);
// wildcard scores 0; a repeated letter ("ACGTA", :248) maps to its last position.
extern "C" parasail_matrix_t *parasail_matrix_create(const char *alphabet, const int match, const int mismatch)
{
    if (!alphabet || !*alphabet) return nullptr;
    MatrixBox *b = new MatrixBox;
    b->alphabet = std::string(alphabet) + "*";
    b->name = "";
    const int n = (int)strlen(alphabet), size = n + 1;
    b->scores.assign((size_t)size * size, 0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) b->scores[(size_t)i * size + j] = (i == j) ? match : mismatch;
    fill_mapper(b->mapper, alphabet, n);
    finish_box(b, PARASAIL_MATRIX_TYPE_SQUARE, size, size, true);
    return publish(b);
}

static parasail_matrix_t g_blosum62, g_nuc44;
static std::vector<int> g_blosum62_mapper, g_nuc44_mapper;
static std::once_flag g_builtin_once;
static void init_builtins()
{
    fill_mapper(g_blosum62_mapper, std::string(pmx_blosum62_alphabet, 23), 23);
    g_blosum62_mapper[(unsigned char)'*'] = 23;
    g_blosum62.name = "blosum62";
    g_blosum62.matrix = pmx_blosum62_scores;
    g_blosum62.mapper = g_blosum62_mapper.data();
    g_blosum62.size = 24; g_blosum62.max = 11; g_blosum62.min = -4;
    g_blosum62.user_matrix = nullptr; g_blosum62.type = PARASAIL_MATRIX_TYPE_SQUARE;
    g_blosum62.length = 24; g_blosum62.alphabet = pmx_blosum62_alphabet; g_blosum62.query = nullptr;
    fill_mapper(g_nuc44_mapper, std::string(pmx_nuc44_alphabet, 15), 15);
    g_nuc44_mapper[(unsigned char)'*'] = 15;
    g_nuc44.name = "nuc44"; g_nuc44.matrix = pmx_nuc44_scores; g_nuc44.mapper = g_nuc44_mapper.data();
    g_nuc44.size = 16; g_nuc44.max = 5; g_nuc44.min = -5; g_nuc44.user_matrix = nullptr;
    g_nuc44.type = PARASAIL_MATRIX_TYPE_SQUARE; g_nuc44.length = 16; g_nuc44.alphabet = pmx_nuc44_alphabet; g_nuc44.query = nullptr;
}

extern "C" parasail_matrix_t *parasail_matrix_from_file(const char *filename);
extern "C" void parasail_matrix_free(parasail_matrix_t *matrix);

// The reference documents 66 built-in names (blosum{30..100}, pam{10..500}: src/matrix/mod.rs:46-50); the tables themselves live in
// the parasail C library, which is not in this image, and typing 64 of them from memory cannot be checked here.  Embedded:
// blosum62, nuc44 (both verified against files: tests/golden/blosum62.txt, the reference's own tests/square.txt).  Every other
// name resolves from $PMX_MATRIX_DIR/<name>[.txt|.mat] (NCBI format, the loader of parasail_matrix_from_file) and then
// behaves like a built-in: cached for the life of the process, never freed, set_value rejected.
//
// ONE table of the documented names with what their files must look like: the 20 residues + B Z X * of the NCBI files
// (24 symbols; a file with further columns, e.g. J / U / O of newer NCBI releases, is accepted as long as these are there).
static const char *const pmx_documented_residues = "ARNDCQEGHILKMFPSTWYV";
static bool documented_matrix_name(const std::string &lname, std::string *family)
{
    static const int blosum[] = {30, 35, 40, 45, 50, 55, 60, 62, 65, 70, 75, 80, 85, 90, 95, 100};
    auto number = [&](const char *prefix, int *out) {
        const size_t pl = strlen(prefix);
        if (lname.compare(0, pl, prefix) != 0 || lname.size() == pl || lname.size() > pl + 3) return false;
        int v = 0;
        for (size_t i = pl; i < lname.size(); ++i) { if (!isdigit((unsigned char)lname[i])) return false; v = 10 * v + (lname[i] - '0'); }
        if (lname[pl] == '0') return false;
        *out = v; return true;
    };
    int v = 0;
    if (number("blosum", &v)) { for (int b : blosum) if (b == v) { if (family) *family = "blosum"; return true; } return false; }
    if (number("pam", &v)) { if (v >= 10 && v <= 500 && v % 10 == 0) { if (family) *family = "pam"; return true; } return false; }
    return false;
}
// the 66 names, for tests and for `pmx_last_error()` ("known name, file missing" vs "unknown name")
extern "C" int pmx_documented_matrix_names(char *buf, int cap)
{
    std::string all;
    static const int blosum[] = {30, 35, 40, 45, 50, 55, 60, 62, 65, 70, 75, 80, 85, 90, 95, 100};
    for (int b : blosum) all += "blosum" + std::to_string(b) + "\n";
    for (int p = 10; p <= 500; p += 10) all += "pam" + std::to_string(p) + "\n";
    if (buf && cap > 0) { strncpy(buf, all.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
    return (int)all.size() + 1;
}

// Load-time self-check of a file that claims a documented name: a damaged or mislabelled table is refused (a silently wrong table
// is worse than a failed lookup).  Square; the 20 residues, B, Z, X and * present; symmetric; positive diagonal on the residues;
// every `*` score against a letter is the table's minimum; B lies between N and D, Z between Q and E, X inside the residues' range.
static bool documented_matrix_selfcheck(const parasail_matrix_t *m, std::string *why)
{
    if (m->type != PARASAIL_MATRIX_TYPE_SQUARE) { *why = "not a square matrix"; return false; }
    const int n = m->size;
    auto idx = [&](char c) -> int { const char *p = m->alphabet ? strchr(m->alphabet, c) : nullptr; return p ? (int)(p - m->alphabet) : -1; };
    auto at = [&](int a, int b) { return m->matrix[(size_t)a * n + b]; };
    int res[20];
    for (int r = 0; r < 20; ++r) { res[r] = idx(pmx_documented_residues[r]); if (res[r] < 0) { *why = std::string("residue ") + pmx_documented_residues[r] + " missing"; return false; } }
    const int iB = idx('B'), iZ = idx('Z'), iX = idx('X'), iS = idx('*');
    if (iB < 0 || iZ < 0 || iX < 0 || iS < 0) { *why = "one of B Z X * missing"; return false; }
    for (int a = 0; a < n; ++a) for (int b = 0; b < a; ++b) if (at(a, b) != at(b, a)) {
        *why = std::string("not symmetric at ") + m->alphabet[a] + "/" + m->alphabet[b]; return false; }
    for (int r = 0; r < 20; ++r) if (at(res[r], res[r]) <= 0) { *why = std::string("diagonal of ") + pmx_documented_residues[r] + " is not positive"; return false; }
    for (int a = 0; a < n; ++a) if (a != iS && at(iS, a) != m->min) { *why = std::string("* against ") + m->alphabet[a] + " is not the table's minimum"; return false; }
    auto between = [&](int amb, char c1, char c2, const char *nm) {
        const int i1 = idx(c1), i2 = idx(c2);
        for (int r = 0; r < 20; ++r) {
            const int lo = std::min(at(i1, res[r]), at(i2, res[r])), hi = std::max(at(i1, res[r]), at(i2, res[r]));
            if (at(amb, res[r]) < lo || at(amb, res[r]) > hi) { *why = std::string(nm) + " against " + pmx_documented_residues[r] + " is outside the range of the residues it stands for"; return false; }
        }
        return true;
    };
    if (!between(iB, 'N', 'D', "B") || !between(iZ, 'Q', 'E', "Z")) return false;
    for (int r = 0; r < 20; ++r) {
        int lo = INT32_MAX, hi = INT32_MIN;
        for (int q = 0; q < 20; ++q) { lo = std::min(lo, at(res[q], res[r])); hi = std::max(hi, at(res[q], res[r])); }
        if (at(iX, res[r]) < lo || at(iX, res[r]) > hi) { *why = std::string("X against ") + pmx_documented_residues[r] + " is outside the residues' range"; return false; }
    }
    return true;
}

static const parasail_matrix_t *lookup_in_matrix_dir(const std::string &lname)
{
    static std::mutex mx;
    static std::unordered_map<std::string, const parasail_matrix_t *> cache;
    for (char c : lname) if (!(isalnum((unsigned char)c) || c == '_' || c == '-' || c == '.')) { set_err("matrix lookup: '%s' is not a name", lname.c_str()); return nullptr; }
    if (lname.empty() || lname[0] == '.') { set_err("matrix lookup: empty name"); return nullptr; }
    const bool documented = documented_matrix_name(lname, nullptr);
    std::lock_guard<std::mutex> lk(mx);
    // $PMX_MATRIX_DIR, else the directory shipped beside the library: <libdir>/../matrices (parasail-rs_amd/matrices in this tree)
    std::string dir;
    const char *env = pmx_env("PMX_MATRIX_DIR");
    if (env && *env) dir = env;
    else {
        Dl_info info;
        if (dladdr((const void *)&lookup_in_matrix_dir, &info) && info.dli_fname) {
            const std::string so(info.dli_fname);
            const size_t slash = so.rfind('/');
            dir = (slash == std::string::npos ? std::string(".") : so.substr(0, slash)) + "/../matrices";
        }
    }
    if (dir.empty()) { set_err("matrix lookup: no matrix directory"); return nullptr; }
    const std::string key = dir + "\n" + lname;               // hits are remembered per directory; a miss is looked up again (a file may have arrived)
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    parasail_matrix_t *m = nullptr;
    for (const char *suffix : {"", ".txt", ".mat"}) {
        const std::string path = dir + "/" + lname + suffix;
        m = parasail_matrix_from_file(path.c_str());
        if (m) break;
    }
    if (!m) {
        if (documented) set_err("matrix lookup: '%s' is a documented name (src/matrix/mod.rs:46-50) whose table is not embedded, and no file %s/%s[.txt|.mat] "
                                "was found: put the NCBI file there (or set PMX_MATRIX_DIR)", lname.c_str(), dir.c_str(), lname.c_str());
        else set_err("matrix lookup: unknown matrix name '%s' (not embedded, not documented, no file in %s)", lname.c_str(), dir.c_str());
        return nullptr;
    }
    if (documented) {
        std::string why;
        if (!documented_matrix_selfcheck(m, &why)) {
            set_err("matrix lookup: the file found for '%s' in %s is refused: %s", lname.c_str(), dir.c_str(), why.c_str());
            parasail_matrix_free(m);
            return nullptr;
        }
    }
    MatrixBox *b = nullptr;
    {   // from here on it is a built-in: out of the table of caller-owned matrices, not writable
        std::lock_guard<std::mutex> lk2(g_mx_mutex);
        auto bi = g_boxes.find(m);
        if (bi != g_boxes.end()) { b = bi->second; g_boxes.erase(bi); }
    }
    if (b) { b->name = lname; b->m.name = b->name.c_str(); }
    m->user_matrix = nullptr;
    cache[key] = m;
    return m;
}

// src/matrix/mod.rs:57-73: NULL -> Error::FailedLookup.  Built-ins are static, never freed.
extern "C" const parasail_matrix_t *parasail_matrix_lookup(const char *matrixname)
{
    if (!matrixname) return nullptr;
    std::call_once(g_builtin_once, init_builtins);
    std::string s(matrixname);
    for (auto &c : s) c = (char)tolower((unsigned char)c);
    if (s == "blosum62") return &g_blosum62;
    if (s == "nuc44" || s == "dnafull") return &g_nuc44;      // EDNAFULL is the NUC.4.4 table under EMBOSS's name
    return lookup_in_matrix_dir(s);
}

// File formats: tests/square.txt:1-27 (square, trailing wildcard row/col) and
// tests/pssm.txt:1-17 (PSSM, optional leading residue column).
extern "C" parasail_matrix_t *parasail_matrix_from_file(const char *filename)
{
    if (!filename) return nullptr;
    FILE *fh = fopen(filename, "r");
    if (!fh) return nullptr;
    std::vector<std::string> header;
    std::vector<std::vector<std::string>> rows;
    char line[8192];
    while (fgets(line, sizeof line, fh)) {
        char *p = line;
        while (*p && isspace((unsigned char)*p)) ++p;
        if (!*p || *p == '#') continue;
        std::vector<std::string> tok;
        char *save = nullptr;
        for (char *t = strtok_r(p, " \t\r\n", &save); t; t = strtok_r(nullptr, " \t\r\n", &save)) tok.emplace_back(t);
        if (tok.empty()) continue;
        if (header.empty()) header = tok; else rows.push_back(tok);
    }
    fclose(fh);
    const int n = (int)header.size();
    if (n < 2 || rows.empty()) return nullptr;
    for (auto &h : header) if (h.size() != 1) return nullptr;
    bool square = (int)rows.size() == n;
    if (square) for (int i = 0; i < n; ++i)
        if ((int)rows[i].size() != n + 1 || rows[i][0] != header[i]) { square = false; break; }
    MatrixBox *b = new MatrixBox;
    b->name = filename;
    for (auto &h : header) b->alphabet += h;
    auto parse = [](const std::string &s, int *out) {
        char *end = nullptr; long v = strtol(s.c_str(), &end, 10);
        if (!end || *end) return false; *out = (int)v; return true;
    };
    if (square) {
        b->scores.resize((size_t)n * n);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j)
            if (!parse(rows[i][j + 1], &b->scores[(size_t)i * n + j])) { delete b; return nullptr; }
        fill_mapper(b->mapper, b->alphabet.substr(0, n - 1), n - 1);
        b->mapper[(unsigned char)b->alphabet[n - 1]] = n - 1;
        finish_box(b, PARASAIL_MATRIX_TYPE_SQUARE, n, n, true);
    } else {
        const int len = (int)rows.size(), size = n + 1;
        b->scores.assign((size_t)len * size, 0);
        for (int i = 0; i < len; ++i) {
            const int skip = (int)rows[i].size() == n + 1 ? 1 : 0;
            if ((int)rows[i].size() != n + skip) { delete b; return nullptr; }
            int mn = INT32_MAX;
            for (int j = 0; j < n; ++j) {
                int v; if (!parse(rows[i][j + skip], &v)) { delete b; return nullptr; }
                b->scores[(size_t)i * size + j] = v; mn = v < mn ? v : mn;
            }
            b->scores[(size_t)i * size + n] = mn;
            if (skip) b->query += rows[i][0];
        }
        b->alphabet += "*";
        fill_mapper(b->mapper, b->alphabet.substr(0, n), n);
        finish_box(b, PARASAIL_MATRIX_TYPE_PSSM, len, size, true);
    }
    return publish(b);
}

// src/matrix/mod.rs:154-169: `values` holds length * strlen(alphabet) scores, row-major.
extern "C" parasail_matrix_t *parasail_matrix_pssm_create(const char *alphabet, const int *values, const int length)
{
    if (!alphabet || !*alphabet || !values || length <= 0) return nullptr;
    const int n = (int)strlen(alphabet), size = n + 1;
    MatrixBox *b = new MatrixBox;
    b->alphabet = std::string(alphabet) + "*";
    b->scores.assign((size_t)length * size, 0);
    for (int i = 0; i < length; ++i) {
        int mn = INT32_MAX;
        for (int j = 0; j < n; ++j) { const int v = values[(size_t)i * n + j]; b->scores[(size_t)i * size + j] = v; mn = v < mn ? v : mn; }
        b->scores[(size_t)i * size + n] = mn;
    }
    fill_mapper(b->mapper, alphabet, n);
    finish_box(b, PARASAIL_MATRIX_TYPE_PSSM, length, size, true);
    return publish(b);
}

// src/matrix/mod.rs:180-212
extern "C" parasail_matrix_t *parasail_matrix_convert_square_to_pssm(const parasail_matrix_t *matrix,
                                                                   const char *s1, int s1Len)
{
    if (!matrix || matrix->type != PARASAIL_MATRIX_TYPE_SQUARE || !s1 || s1Len <= 0) return nullptr;
    MatrixBox *b = new MatrixBox;
    b->name = matrix->name ? matrix->name : "";
    b->alphabet = matrix->alphabet ? matrix->alphabet : "";
    b->query.assign(s1, (size_t)s1Len);
    const int size = matrix->size;
    b->scores.resize((size_t)s1Len * size);
    for (int i = 0; i < s1Len; ++i)
        memcpy(&b->scores[(size_t)i * size], &matrix->matrix[(size_t)matrix->mapper[(unsigned char)s1[i]] * size],
               sizeof(int) * (size_t)size);
    b->mapper.assign(matrix->mapper, matrix->mapper + 256);
    finish_box(b, PARASAIL_MATRIX_TYPE_PSSM, s1Len, size, true);
    return publish(b);
}

// src/matrix/mod.rs:279-294
extern "C" parasail_matrix_t *parasail_matrix_copy(const parasail_matrix_t *matrix)
{
    if (!matrix) return nullptr;
    MatrixBox *b = new MatrixBox;
    b->name = matrix->name ? matrix->name : "";
    b->alphabet = matrix->alphabet ? matrix->alphabet : "";
    if (matrix->query) b->query = matrix->query;
    b->scores.assign(matrix->matrix, matrix->matrix + (size_t)matrix->length * matrix->size);
    b->mapper.assign(matrix->mapper, matrix->mapper + 256);
    finish_box(b, matrix->type, matrix->length, matrix->size, true);
    return publish(b);
}

static void devcache_drop(const parasail_matrix_t *m);

// src/matrix/mod.rs:222-242 (Rust checks the index range and the builtin flag first)
extern "C" void parasail_matrix_set_value(parasail_matrix_t *matrix, int row, int col, int value)
{
    if (!matrix || !matrix->user_matrix) return;
    if (row < 0 || col < 0 || row >= matrix->length || col >= matrix->size) return;
    matrix->user_matrix[(size_t)row * matrix->size + col] = value;
    if (value > matrix->max) matrix->max = value;
    if (value < matrix->min) matrix->min = value;
    devcache_drop(matrix);
}

// src/matrix/mod.rs:297-307
extern "C" void parasail_matrix_free(parasail_matrix_t *matrix)
{
    if (!matrix) return;
    MatrixBox *b = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mx_mutex);
        auto it = g_boxes.find(matrix);
        if (it == g_boxes.end()) return;       // builtin or unknown: never freed
        b = it->second; g_boxes.erase(it);
    }
    devcache_drop(matrix);
    delete b;
}

// ===================================================================== device matrices ===
struct DevMat { PmxDevMatrix d; int16_t *scores; uint8_t *mapper; uint64_t hash; int rows; };
static std::mutex g_dev_mutex;
static std::unordered_map<uint64_t, DevMat> g_devmats;     // key = matrix ptr ^ device

static uint64_t mat_hash(const parasail_matrix_t *m)
{
    uint64_t h = 1469598103934665603ULL;
    auto mix = [&](int v) { h ^= (uint32_t)v; h *= 1099511628211ULL; };
    const size_t cells = (size_t)m->length * m->size;
    for (size_t i = 0; i < cells; ++i) mix(m->matrix[i]);
    for (int i = 0; i < 256; ++i) mix(m->mapper[i]);
    mix(m->size); mix(m->length); mix(m->type);
    return h;
}

static void devcache_drop(const parasail_matrix_t *m)
{
    std::lock_guard<std::mutex> lk(g_dev_mutex);
    for (auto it = g_devmats.begin(); it != g_devmats.end();) {
        if ((it->first >> 8) == ((uint64_t)(uintptr_t)m)) {
            (void)hipFree(it->second.scores); (void)hipFree(it->second.mapper);
            it = g_devmats.erase(it);
        } else ++it;
    }
}

// Upload (once per matrix content and device) the int16 score table + byte mapper.
static int get_devmat(const parasail_matrix_t *m, DevMat *out)
{
    if (!m || !m->matrix || !m->mapper || m->size <= 0 || m->size > 255) { set_err("bad matrix"); return -1; }
    if (m->max > 32767 || m->min < -32768) { set_err("matrix scores do not fit int16"); return -1; }
    int dev = 0; HIP_OR_RET(hipGetDevice(&dev));
    const uint64_t key = ((uint64_t)(uintptr_t)m << 8) | (uint64_t)(dev & 0xFF);
    const uint64_t h = mat_hash(m);
    std::lock_guard<std::mutex> lk(g_dev_mutex);
    auto it = g_devmats.find(key);
    if (it != g_devmats.end() && it->second.hash == h) { *out = it->second; return 0; }
    if (it != g_devmats.end()) { (void)hipFree(it->second.scores); (void)hipFree(it->second.mapper); g_devmats.erase(it); }
    const size_t cells = (size_t)m->length * m->size;
    std::vector<int16_t> s16(cells); std::vector<uint8_t> map8(256);
    for (size_t i = 0; i < cells; ++i) s16[i] = (int16_t)m->matrix[i];
    for (int i = 0; i < 256; ++i) {
        int v = m->mapper[i];
        if (v < 0 || v >= m->size) v = m->size - 1;
        map8[i] = (uint8_t)v;
    }
    DevMat dm; dm.hash = h; dm.rows = m->length;
    HIP_OR_RET(hipMalloc(&dm.scores, cells * 2));
    HIP_OR_RET(hipMalloc(&dm.mapper, 256));
    HIP_OR_RET(hipMemcpy(dm.scores, s16.data(), cells * 2, hipMemcpyHostToDevice));
    HIP_OR_RET(hipMemcpy(dm.mapper, map8.data(), 256, hipMemcpyHostToDevice));
    dm.d.scores = dm.scores; dm.d.mapper = dm.mapper; dm.d.msize = m->size; dm.d.min = m->min; dm.d.max = m->max;
    dm.d.pssm = m->type == PARASAIL_MATRIX_TYPE_PSSM ? 1 : 0; dm.d.rows = dm.d.pssm ? m->length : m->size;
    g_devmats[key] = dm;
    *out = dm;
    return 0;
}

// ============================================================================ results ====
enum {
    F_NW = 1 << 0, F_SG = 1 << 1, F_SW = 1 << 2, F_SATURATED = 1 << 6, F_BANDED = 1 << 7,
    F_SCAN = 1 << 10, F_STRIPED = 1 << 11, F_DIAG = 1 << 12, F_BLOCKED = 1 << 13,
    F_STATS = 1 << 16, F_TABLE = 1 << 17, F_ROWCOL = 1 << 18, F_TRACE = 1 << 19,
    F_BITS_8 = 1 << 20, F_BITS_16 = 1 << 21, F_BITS_32 = 1 << 22, F_BITS_64 = 1 << 23
};

struct PmxPendQueue;
struct parasail_result {
    int score, end_query, end_ref, flag;
    int matches, similar, length;
    int qlen, rlen;
    int *tables[4];        // score, matches, similar, length  [qlen*rlen]
    int *rows[4];          // [rlen]
    int *cols[4];          // [qlen]
    int8_t *trace;         // [qlen*rlen]
    // Deferred results (switch PMX_DEFER_ALIGN): non-null while the pair sits in a queue of calls that have not run yet; the first
    // accessor that needs a computed field (of ANY result of that queue) runs the whole queue as one batch.  A heap block holding a
    // shared reference to the queue, so that a result may be read or freed from another thread and outlives its creator thread.
    struct PmxPendRef *pending;
};
static void pend_resolve(const parasail_result_t *r);
#define RESOLVE(r) do { if (__atomic_load_n(&(r)->pending, __ATOMIC_ACQUIRE)) pend_resolve(r); } while (0)

extern "C" {
int parasail_result_get_score(const parasail_result_t *r) { RESOLVE(r); return r->score; }
int parasail_result_get_end_query(const parasail_result_t *r) { RESOLVE(r); return r->end_query; }
int parasail_result_get_end_ref(const parasail_result_t *r) { RESOLVE(r); return r->end_ref; }
int parasail_result_get_matches(const parasail_result_t *r) { RESOLVE(r); return r->matches; }
int parasail_result_get_similar(const parasail_result_t *r) { RESOLVE(r); return r->similar; }
int parasail_result_get_length(const parasail_result_t *r) { RESOLVE(r); return r->length; }
int *parasail_result_get_score_table(const parasail_result_t *r) { return r->tables[0]; }
int *parasail_result_get_matches_table(const parasail_result_t *r) { return r->tables[1]; }
int *parasail_result_get_similar_table(const parasail_result_t *r) { return r->tables[2]; }
int *parasail_result_get_length_table(const parasail_result_t *r) { return r->tables[3]; }
int *parasail_result_get_score_row(const parasail_result_t *r) { return r->rows[0]; }
int *parasail_result_get_matches_row(const parasail_result_t *r) { return r->rows[1]; }
int *parasail_result_get_similar_row(const parasail_result_t *r) { return r->rows[2]; }
int *parasail_result_get_length_row(const parasail_result_t *r) { return r->rows[3]; }
int *parasail_result_get_score_col(const parasail_result_t *r) { return r->cols[0]; }
int *parasail_result_get_matches_col(const parasail_result_t *r) { return r->cols[1]; }
int *parasail_result_get_similar_col(const parasail_result_t *r) { return r->cols[2]; }
int *parasail_result_get_length_col(const parasail_result_t *r) { return r->cols[3]; }
int *parasail_result_get_trace_table(const parasail_result_t *r) { return reinterpret_cast<int *>(r->trace); }
int parasail_result_is_nw(const parasail_result_t *r) { return !!(r->flag & F_NW); }
int parasail_result_is_sg(const parasail_result_t *r) { return !!(r->flag & F_SG); }
int parasail_result_is_sw(const parasail_result_t *r) { return !!(r->flag & F_SW); }
int parasail_result_is_saturated(const parasail_result_t *r) { RESOLVE(r); return !!(r->flag & F_SATURATED); }
int parasail_result_is_banded(const parasail_result_t *r) { return !!(r->flag & F_BANDED); }
int parasail_result_is_scan(const parasail_result_t *r) { return !!(r->flag & F_SCAN); }
int parasail_result_is_striped(const parasail_result_t *r) { return !!(r->flag & F_STRIPED); }
int parasail_result_is_diag(const parasail_result_t *r) { return !!(r->flag & F_DIAG); }
int parasail_result_is_blocked(const parasail_result_t *r) { return !!(r->flag & F_BLOCKED); }
int parasail_result_is_stats(const parasail_result_t *r) { return !!(r->flag & F_STATS); }
/* tests/test_parasail.rs:276-279, :397-399: stats+table -> is_table && is_stats && is_stats_table */
int parasail_result_is_stats_table(const parasail_result_t *r) { return (r->flag & F_STATS) && (r->flag & F_TABLE); }
int parasail_result_is_table(const parasail_result_t *r) { return !!(r->flag & F_TABLE); }
int parasail_result_is_rowcol(const parasail_result_t *r) { return !!(r->flag & F_ROWCOL); }
int parasail_result_is_stats_rowcol(const parasail_result_t *r) { return (r->flag & F_STATS) && (r->flag & F_ROWCOL); }
int parasail_result_is_trace(const parasail_result_t *r) { return !!(r->flag & F_TRACE); }

static void pend_cancel(parasail_result_t *r);
void parasail_result_free(parasail_result_t *r)
{
    if (!r) return;
    if (__atomic_load_n(&r->pending, __ATOMIC_ACQUIRE)) pend_cancel(r);      // a result that was never looked at: its pair leaves the queue
    for (int k = 0; k < 4; ++k) { free(r->tables[k]); free(r->rows[k]); free(r->cols[k]); }
    free(r->trace);
    free(r);
}
}  // extern "C"

// ====================================================================== single-pair run ===
struct RunSpec {
    int mode, sg_flags, band;
    int width;             // 0 sat, 8, 16, 32, 64
    bool stats, table, rowcol, trace;
    int vecflag;           // F_STRIPED / F_SCAN / F_DIAG / 0
};

static int run_batch_device(const pmx_config_t *cfg, int64_t n,
                            const uint8_t *d_qbuf, const int64_t *d_qoff, int q_shared,
                            const uint8_t *d_rbuf, const int64_t *d_roff,
                            int32_t max_qlen, int32_t max_rlen,
                            pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream, int q_shared_wild = 1);

// One device block + one pinned host block per thread for the one-pair entry: a single H2D, the
// kernel(s), a single D2H.  (The reference's call is a CPU function of ~20 us; no allocation per call.)
struct SingleWs { void *dev = nullptr; void *pin = nullptr; size_t cap = 0; int device = -1; void *big = nullptr; size_t bigcap = 0; int bigdev = -1;
                  hipStream_t stream = nullptr; int streamdev = -1; };      // (a stream per host thread: one-pair calls of several threads overlap on the chip)
static thread_local SingleWs g_single;
// one device block per host thread for the one-pair calls that return tables (carved up per call: a dozen hipMalloc / hipFree
// per call cost more than the kernel)
// The block is kept between calls only up to SINGLE_BIG_KEEP: one 20 kbp x 20 kbp table call would otherwise pin gigabytes of HBM
// per host thread for the life of the process (the batch entries size their chunks from the free memory they find).
static const size_t SINGLE_BIG_KEEP = (size_t)256 << 20;
static void single_big_reserve(size_t bytes)
{
    int dev = 0; HIP_OR_DIE(hipGetDevice(&dev));
    if (g_single.bigdev == dev && g_single.bigcap >= bytes) return;
    if (g_single.big) (void)hipFree(g_single.big);
    g_single.big = nullptr; g_single.bigcap = 0; g_single.bigdev = -1;
    const size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 2 <= SINGLE_BIG_KEEP ? bytes + bytes / 2 : bytes;
    HIP_OR_DIE(hipMalloc(&g_single.big, cap));
    g_single.bigcap = cap; g_single.bigdev = dev;
}
static void single_big_trim()
{
    if (g_single.big && g_single.bigcap > SINGLE_BIG_KEEP) {
        (void)hipFree(g_single.big);
        g_single.big = nullptr; g_single.bigcap = 0; g_single.bigdev = -1;
    }
}
static void single_reserve(size_t bytes)
{
    int dev = 0; HIP_OR_DIE(hipGetDevice(&dev));
    if (g_single.streamdev != dev) {
        // the reference's parallel story is threads calling align() side by side (tests/test_parasail.rs:689-723): on the legacy default
        // stream their launches would run one after the other (20 k pairs/s whatever the thread count, profiles/r04/thread_table.txt)
        if (g_single.stream) (void)hipStreamDestroy(g_single.stream);
        HIP_OR_DIE(hipStreamCreateWithFlags(&g_single.stream, hipStreamNonBlocking));
        g_single.streamdev = dev;
    }
    if (g_single.device == dev && g_single.cap >= bytes) return;
    if (g_single.dev) { (void)hipFree(g_single.dev); (void)hipHostFree(g_single.pin); }
    const size_t cap = bytes < 65536 ? 65536 : bytes * 2;
    HIP_OR_DIE(hipMalloc(&g_single.dev, cap));
    HIP_OR_DIE(hipHostMalloc(&g_single.pin, cap, hipHostMallocDefault));
    g_single.cap = cap; g_single.device = dev;
}

template <typename T> struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void alloc(size_t n) { HIP_OR_DIE(hipMalloc(&p, (n ? n : 1) * sizeof(T))); }
    int try_alloc(size_t n) { return hipMalloc(&p, (n ? n : 1) * sizeof(T)) == hipSuccess ? 0 : -1; }   // entries that can report an error
};

// ---- deferred results (PMX_DEFER_ALIGN) ----------------------------------------------------------------------------------
// One queue per host thread and configuration: packed sequences as the batch entry wants them, and the results waiting for them.
struct PmxPendQueue {
    std::mutex mx;
    pmx_config_t cfg; RunSpec sp;
    std::vector<uint8_t> qbuf, rbuf;
    std::vector<int64_t> qoff{0}, roff{0};
    std::vector<parasail_result_t *> res;          // nullptr: the result was freed before anything asked for it
};
struct PmxPendRef { std::shared_ptr<PmxPendQueue> q; };
static thread_local std::shared_ptr<PmxPendQueue> g_pend;

extern "C" int pmx_align_batch(const pmx_config_t *cfg, int64_t n, const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                               pmx_record_t *out, pmx_stats_t *stats_out);

// runs the queue (its mutex held by the caller) and completes every result in it
static void pend_flush_locked(PmxPendQueue &q)
{
    const int64_t n = (int64_t)q.res.size();
    if (!n) return;
    std::vector<pmx_record_t> rec((size_t)n);
    std::vector<pmx_stats_t> st(q.sp.stats ? (size_t)n : 0);
    if (pmx_align_batch(&q.cfg, n, q.qbuf.data(), q.qoff.data(), q.rbuf.data(), q.roff.data(), rec.data(), q.sp.stats ? st.data() : nullptr))
        die(g_err, hipSuccess);
    for (int64_t k = 0; k < n; ++k) {
        parasail_result_t *r = q.res[(size_t)k];
        if (!r) continue;
        r->score = rec[(size_t)k].score; r->end_query = rec[(size_t)k].end_query; r->end_ref = rec[(size_t)k].end_ref;
        if (rec[(size_t)k].flags & PMX_FLAG_SATURATED) r->flag |= F_SATURATED;
        if (q.sp.stats) { r->matches = st[(size_t)k].matches; r->similar = st[(size_t)k].similar; r->length = st[(size_t)k].length; }
        PmxPendRef *ref = r->pending;
        __atomic_store_n(&r->pending, (PmxPendRef *)nullptr, __ATOMIC_RELEASE);
        delete ref;
    }
    q.qbuf.clear(); q.rbuf.clear(); q.qoff.assign(1, 0); q.roff.assign(1, 0); q.res.clear();
}
static void pend_resolve(const parasail_result_t *r)
{
    PmxPendRef *ref = __atomic_load_n(&r->pending, __ATOMIC_ACQUIRE);
    if (!ref) return;
    std::shared_ptr<PmxPendQueue> q = ref->q;          // (the flush deletes `ref`)
    std::lock_guard<std::mutex> lk(q->mx);
    if (__atomic_load_n(&r->pending, __ATOMIC_ACQUIRE)) pend_flush_locked(*q);
}
static void pend_cancel(parasail_result_t *r)
{
    PmxPendRef *ref = __atomic_load_n(&r->pending, __ATOMIC_ACQUIRE);
    if (!ref) return;
    std::shared_ptr<PmxPendQueue> q = ref->q;
    std::lock_guard<std::mutex> lk(q->mx);
    ref = __atomic_load_n(&r->pending, __ATOMIC_ACQUIRE);
    if (!ref) return;                                   // completed meanwhile
    for (auto &p : q->res) if (p == r) { p = nullptr; break; }     // its pair still runs with the batch; nobody reads the record
    __atomic_store_n(&r->pending, (PmxPendRef *)nullptr, __ATOMIC_RELEASE);
    delete ref;
}
// true: the pair was queued and `res` is pending
static bool pend_enqueue(parasail_result_t *res, const RunSpec &sp, const char *s1, int s1Len, const char *s2, int s2Len,
                         int open, int gap, const parasail_matrix_t *matrix)
{
    if (!pmx_env("PMX_DEFER_ALIGN")) return false;
    if ((long long)s1Len * s2Len > (1LL << 20)) return false;           // long pairs fill the chip on their own
    if (!g_pend) g_pend = std::make_shared<PmxPendQueue>();
    std::shared_ptr<PmxPendQueue> q = g_pend;
    std::lock_guard<std::mutex> lk(q->mx);
    const bool same = !q->res.empty() && q->sp.mode == sp.mode && q->sp.sg_flags == sp.sg_flags && q->sp.width == sp.width &&
                      q->sp.stats == sp.stats && q->cfg.open == open && q->cfg.extend == gap && q->cfg.matrix == matrix;
    if (!q->res.empty() && (!same || q->res.size() >= (1u << 18) || q->qbuf.size() + q->rbuf.size() > ((size_t)256 << 20)))
        pend_flush_locked(*q);                                           // another configuration, or enough for one batch
    if (q->res.empty()) {
        q->sp = sp; memset(&q->cfg, 0, sizeof q->cfg);
        q->cfg.mode = sp.mode; q->cfg.sg_flags = sp.sg_flags; q->cfg.open = open; q->cfg.extend = gap; q->cfg.width = sp.width;
        q->cfg.want = sp.stats ? PMX_WANT_STATS : 0; q->cfg.matrix = matrix;
    }
    q->qbuf.insert(q->qbuf.end(), (const uint8_t *)s1, (const uint8_t *)s1 + s1Len);
    q->rbuf.insert(q->rbuf.end(), (const uint8_t *)s2, (const uint8_t *)s2 + s2Len);
    q->qoff.push_back((int64_t)q->qbuf.size()); q->roff.push_back((int64_t)q->rbuf.size());
    q->res.push_back(res);
    PmxPendRef *ref = new PmxPendRef{q};
    __atomic_store_n(&res->pending, ref, __ATOMIC_RELEASE);
    return true;
}
// every pending result of the calling thread's queue, now (the mirrors call it when an aligner that deferred work goes away)
extern "C" void pmx_flush_deferred(void)
{
    if (!g_pend) return;
    std::shared_ptr<PmxPendQueue> q = g_pend;
    std::lock_guard<std::mutex> lk(q->mx);
    pend_flush_locked(*q);
}

static parasail_result_t *run_single(const RunSpec &sp, const char *s1, int s1Len, const char *s2, int s2Len,
                                     int open, int gap, const parasail_matrix_t *matrix)
{
    parasail_result_t *res = (parasail_result_t *)calloc(1, sizeof(parasail_result_t));
    if (!res) die("calloc", hipSuccess);
    res->qlen = s1Len; res->rlen = s2Len;
    int flag = sp.vecflag;
    flag |= sp.mode == PMX_MODE_NW ? F_NW : sp.mode == PMX_MODE_SG ? F_SG : F_SW;
    if (sp.band >= 0) flag |= F_BANDED;
    if (sp.stats) flag |= F_STATS;
    if (sp.table) flag |= F_TABLE;
    if (sp.rowcol) flag |= F_ROWCOL;
    if (sp.trace) flag |= F_TRACE;
    flag |= sp.width == 8 ? F_BITS_8 : sp.width == 16 ? F_BITS_16 : sp.width == 64 ? F_BITS_64 : F_BITS_32;
    res->flag = flag;
    if (!s1 || !s2 || s1Len <= 0 || s2Len <= 0 || !matrix) return res;   // degenerate: empty result, never NULL

    const bool pssm = matrix->type == PARASAIL_MATRIX_TYPE_PSSM;
    if (pssm && matrix->length != s1Len) die("PSSM length differs from the query length", hipSuccess);
    // Deferred results (PMX_DEFER_ALIGN): the reference's parallel story is user threads calling align() one pair at a time
    // (tests/test_parasail.rs:689-723); one launch + one wait per 150 x 150 pair is 50 us -- slower than one CPU core.  With the
    // switch on, the call only queues the pair and hands back a PENDING result; the first accessor runs the thread's queue as ONE batch.
    if (!sp.table && !sp.rowcol && !sp.trace && sp.band < 0 && !pssm && pend_enqueue(res, sp, s1, s1Len, s2, s2Len, open, gap, matrix)) return res;
    DevMat dm;
    if (get_devmat(matrix, &dm)) die(g_err, hipSuccess);

    if (!sp.table && !sp.rowcol && !sp.trace && sp.band < 0 && !pssm) {
        // score (+ stats) only: a one-pair batch through the same dispatcher as pmx_align_batch_device
        const size_t qpad = ((size_t)s1Len + 7) & ~(size_t)7, rpad = ((size_t)s2Len + 7) & ~(size_t)7;
        const size_t in_bytes = qpad + rpad + 4 * sizeof(int64_t);
        const size_t total = in_bytes + 64;
        single_reserve(total);
        unsigned char *h = (unsigned char *)g_single.pin, *d = (unsigned char *)g_single.dev;
        memcpy(h, s1, (size_t)s1Len); memcpy(h + qpad, s2, (size_t)s2Len);
        const int64_t offs[4] = {0, s1Len, 0, s2Len};
        memcpy(h + qpad + rpad, offs, sizeof offs);
        // Short pairs: the kernel reads the page-locked staging block itself and writes its record there (the block is mapped into
        // the device's address space), so the call is one launch and one wait -- no copy commands in front of and behind it.
        const bool zero_copy = in_bytes <= 4096;
        if (zero_copy) d = h;
        else HIP_OR_DIE(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, g_single.stream));
        pmx_config_t cfg; memset(&cfg, 0, sizeof cfg);
        cfg.mode = sp.mode; cfg.sg_flags = sp.sg_flags; cfg.open = open; cfg.extend = gap; cfg.width = sp.width;
        cfg.want = sp.stats ? PMX_WANT_STATS : 0; cfg.matrix = matrix;
        pmx_record_t *drec = (pmx_record_t *)(d + in_bytes);
        pmx_stats_t *dst = (pmx_stats_t *)(d + in_bytes + 16);
        const int64_t *doff = (const int64_t *)(d + qpad + rpad);
        if (run_batch_device(&cfg, 1, d, doff, 0, d + qpad, doff + 2, s1Len, s2Len, drec, sp.stats ? dst : nullptr, g_single.stream))
            die(g_err, hipSuccess);
        if (!zero_copy) HIP_OR_DIE(hipMemcpyAsync(h + in_bytes, d + in_bytes, 32, hipMemcpyDeviceToHost, g_single.stream));
        HIP_OR_DIE(hipStreamSynchronize(g_single.stream));
        pmx_record_t rec; pmx_stats_t st;
        memcpy(&rec, h + in_bytes, sizeof rec); memcpy(&st, h + in_bytes + 16, sizeof st);
        res->score = rec.score; res->end_query = rec.end_query; res->end_ref = rec.end_ref;
        if (rec.flags & PMX_FLAG_SATURATED) res->flag |= F_SATURATED;
        if (sp.stats) { res->matches = st.matches; res->similar = st.similar; res->length = st.length; }
        return res;
    }

    const size_t cells = (size_t)s1Len * s2Len;
    const int ntab = sp.stats ? 4 : 1;
    const bool rs_fits = pmx_general_lds_fits(matrix->length, matrix->size, s2Len);
    // one device block, carved up: [q | r | offsets][record, stats][boundary row][mapped reference][tables][rows, columns][trace]
    struct Ptr { void *p = nullptr; };
    struct { uint8_t *p; } dq, dr, drs = {nullptr}; struct { int64_t *p; } doff; struct { pmx_record_t *p; } drec; struct { pmx_stats_t *p; } dst;
    struct { int32_t *p; } dbound, dtab[4] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}}, drow[4] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}},
                           dcol[4] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}};
    struct { int8_t *p; } dtrace = {nullptr};
    const size_t qpad = ((size_t)s1Len + 7) & ~(size_t)7, rpad = ((size_t)s2Len + 7) & ~(size_t)7, in_bytes = qpad + rpad + 4 * sizeof(int64_t);
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t o_in = carve(in_bytes), o_rec = carve(64), o_bound = carve((size_t)8 * s2Len * sizeof(int32_t)),
                 o_rs = rs_fits ? 0 : carve((size_t)s2Len + 32);
    size_t o_tab[4] = {0, 0, 0, 0}, o_row[4] = {0, 0, 0, 0}, o_col[4] = {0, 0, 0, 0}, o_trace = 0;
    if (sp.table) for (int k = 0; k < ntab; ++k) o_tab[k] = carve(cells * sizeof(int32_t));
    if (sp.rowcol) for (int k = 0; k < ntab; ++k) { o_row[k] = carve((size_t)s2Len * sizeof(int32_t)); o_col[k] = carve((size_t)s1Len * sizeof(int32_t)); }
    if (sp.trace) o_trace = carve(cells);
    single_big_reserve(off);
    single_reserve(in_bytes + 64);
    unsigned char *D = (unsigned char *)g_single.big, *h = (unsigned char *)g_single.pin;
    dq.p = D + o_in; dr.p = D + o_in + qpad; doff.p = (int64_t *)(D + o_in + qpad + rpad);
    drec.p = (pmx_record_t *)(D + o_rec); dst.p = (pmx_stats_t *)(D + o_rec + 16);
    dbound.p = (int32_t *)(D + o_bound);
    if (!rs_fits) drs.p = D + o_rs;
    if (sp.table) for (int k = 0; k < ntab; ++k) dtab[k].p = (int32_t *)(D + o_tab[k]);
    if (sp.rowcol) for (int k = 0; k < ntab; ++k) { drow[k].p = (int32_t *)(D + o_row[k]); dcol[k].p = (int32_t *)(D + o_col[k]); }
    if (sp.trace) dtrace.p = (int8_t *)(D + o_trace);
    memcpy(h, s1, (size_t)s1Len); memcpy(h + qpad, s2, (size_t)s2Len);
    const int64_t offs[4] = {0, s1Len, 0, s2Len};
    memcpy(h + qpad + rpad, offs, sizeof offs);
    HIP_OR_DIE(hipMemcpyAsync(D + o_in, h, in_bytes, hipMemcpyHostToDevice, nullptr));

    PmxGeneralArgs a; memset(&a, 0, sizeof a);
    a.qbuf = dq.p; a.qoff = doff.p; a.rbuf = dr.p; a.roff = doff.p + 2; a.n = 1; a.max_rlen = s2Len;
    a.scores = dm.d.scores; a.mapper = dm.d.mapper; a.msize = dm.d.msize;
    a.mat_rows = matrix->length; a.pssm = pssm ? 1 : 0;
    a.mode = sp.mode; a.sg_flags = sp.sg_flags; a.open = open; a.ext = gap; a.band = sp.band;
    a.bits = sp.width; a.max_qlen = s1Len;
    a.bound = dbound.p; a.bound_stride = (long long)8 * s2Len;
    if (!rs_fits) { a.rs_scratch = drs.p; a.rs_stride = (long long)s2Len + 32; }
    a.rec = drec.p; a.stats = dst.p;
    a.score_table = dtab[0].p; a.matches_table = dtab[1].p; a.similar_table = dtab[2].p; a.length_table = dtab[3].p;
    a.score_row = drow[0].p; a.matches_row = drow[1].p; a.similar_row = drow[2].p; a.length_row = drow[3].p;
    a.score_col = dcol[0].p; a.matches_col = dcol[1].p; a.similar_col = dcol[2].p; a.length_col = dcol[3].p;
    a.trace_table = dtrace.p;

    int rc = 1;
    if ((sp.table || sp.rowcol) && !sp.stats && !sp.trace && sp.band < 0 && !pssm && sp.width != 8 && sp.width != 16)
        // score table / last row and column: the row-by-row kernel that writes at HBM speed (pmx_table.hip); widths 8 / 16 keep the
        // general kernel, which reports their saturation
        rc = pmx_launch_table(sp.mode, sp.sg_flags, open, gap, dm.d, 1, dq.p, doff.p, 0, dr.p, doff.p + 2, s1Len, s2Len,
                              nullptr, dtab[0].p, drow[0].p, dcol[0].p, drec.p, nullptr);
    if (rc < 0) die("table kernel launch failed", (hipError_t)(-rc));
    if (sp.trace && !sp.table && !sp.rowcol && !sp.stats && sp.band < 0 && !pssm && sp.width != 8 && sp.width != 16) {
        // trace table alone (use_trace + get_cigar / get_traceback_strings): the same row-by-row kernel writes the bytes
        rc = pmx_launch_table(sp.mode, sp.sg_flags, open, gap, dm.d, 1, dq.p, doff.p, 0, dr.p, doff.p + 2, s1Len, s2Len,
                              nullptr, nullptr, nullptr, nullptr, drec.p, nullptr, dtrace.p);
        if (rc < 0) die("table kernel launch failed", (hipError_t)(-rc));
    }
    if (rc == 1) rc = pmx_launch_general(a, sp.stats, nullptr);
    if (rc) die("general kernel launch failed (matrix too large for LDS?)", hipSuccess);
    pmx_record_t rec; pmx_stats_t st = {0, 0, 0};
    HIP_OR_DIE(hipMemcpyAsync(h + in_bytes, D + o_rec, 32, hipMemcpyDeviceToHost, nullptr));
    HIP_OR_DIE(hipStreamSynchronize(nullptr));
    memcpy(&rec, h + in_bytes, sizeof rec);
    if (sp.stats) memcpy(&st, h + in_bytes + 16, sizeof st);
    res->score = rec.score; res->end_query = rec.end_query; res->end_ref = rec.end_ref;
    if (rec.flags & PMX_FLAG_SATURATED) res->flag |= F_SATURATED;
    res->matches = st.matches; res->similar = st.similar; res->length = st.length;
    auto fetch = [&](int32_t *d, size_t n) -> int * {
        if (!d) return nullptr;
        int *h = (int *)malloc(n * sizeof(int));
        if (!h) die("malloc", hipSuccess);
        HIP_OR_DIE(hipMemcpy(h, d, n * sizeof(int), hipMemcpyDeviceToHost));
        return h;
    };
    for (int k = 0; k < 4; ++k) {
        res->tables[k] = fetch(dtab[k].p, cells);
        res->rows[k] = fetch(drow[k].p, s2Len);
        res->cols[k] = fetch(dcol[k].p, s1Len);
    }
    if (sp.trace) {
        res->trace = (int8_t *)malloc(cells);
        if (!res->trace) die("malloc", hipSuccess);
        HIP_OR_DIE(hipMemcpy(res->trace, dtrace.p, cells, hipMemcpyDeviceToHost));
    }
    single_big_trim();
    return res;
}

// ============================================================== dispatch-name grammar ====
// {mode}{sg_gaps}{trace}{stats}{table}{vec}{profile}_{width}     src/aligner/mod.rs:319-329
// id = ((mode*7 + out)*3 + vec)*5 + width
//   mode : 0 nw, 1 sw, 2 + q*4 + d  (q,d in {none,b,e,x}) for sg
//   out  : 0 -, 1 table, 2 rowcol, 3 stats, 4 stats_table, 5 stats_rowcol, 6 trace
//   vec  : 0 striped, 1 scan, 2 diag          width: 0 sat, 1 8, 2 16, 3 32, 4 64
static const int N_MODE = 18, N_OUT = 7, N_VEC = 3, N_WIDTH = 5;
static const int N_IDS = N_MODE * N_OUT * N_VEC * N_WIDTH;

static RunSpec spec_from_id(int id)
{
    RunSpec sp; memset(&sp, 0, sizeof sp);
    const int w = id % N_WIDTH; id /= N_WIDTH;
    const int v = id % N_VEC; id /= N_VEC;
    const int o = id % N_OUT; id /= N_OUT;
    const int m = id;
    static const int widths[5] = {0, 8, 16, 32, 64};
    sp.width = widths[w];
    sp.vecflag = v == 0 ? F_STRIPED : v == 1 ? F_SCAN : F_DIAG;
    sp.table = (o == 1 || o == 4); sp.rowcol = (o == 2 || o == 5);
    sp.stats = (o >= 3 && o <= 5); sp.trace = (o == 6);
    sp.band = -1;
    if (m == 0) sp.mode = PMX_MODE_NW;
    else if (m == 1) sp.mode = PMX_MODE_SW;
    else {
        sp.mode = PMX_MODE_SG;
        const int qi = (m - 2) / 4, di = (m - 2) % 4;
        int f = 0;
        if (qi == 1 || qi == 3) f |= PMX_SG_QB;
        if (qi == 2 || qi == 3) f |= PMX_SG_QE;
        if (di == 1 || di == 3) f |= PMX_SG_DB;
        if (di == 2 || di == 3) f |= PMX_SG_DE;
        if (qi == 0 && di == 0) f = PMX_SG_ALL;      // plain "sg": every end free
        sp.sg_flags = f;
    }
    return sp;
}

static bool eat(const char *&p, const char *tok)
{
    const size_t n = strlen(tok);
    if (strncmp(p, tok, n) == 0) { p += n; return true; }
    return false;
}

// returns id or -1; *is_profile reports the _profile slot
static int parse_name(const char *name, bool *is_profile)
{
    if (!name) return -1;
    const char *p = name;
    eat(p, "parasail_");
    int m;
    if (eat(p, "nw")) m = 0;
    else if (eat(p, "sw")) m = 1;
    else if (eat(p, "sg")) {
        int qi = 0, di = 0;
        if (eat(p, "_qb")) qi = 1; else if (eat(p, "_qe")) qi = 2; else if (eat(p, "_qx")) qi = 3;
        if (eat(p, "_db")) di = 1; else if (eat(p, "_de")) di = 2; else if (eat(p, "_dx")) di = 3;
        m = 2 + qi * 4 + di;
    } else return -1;
    const bool trace = eat(p, "_trace");
    const bool stats = eat(p, "_stats");
    const bool table = eat(p, "_table");
    const bool rowcol = !table && eat(p, "_rowcol");
    if (trace && (stats || table || rowcol)) return -1;
    int o = trace ? 6 : stats ? (table ? 4 : rowcol ? 5 : 3) : (table ? 1 : rowcol ? 2 : 0);
    int v;
    if (eat(p, "_striped")) v = 0; else if (eat(p, "_scan")) v = 1; else if (eat(p, "_diag")) v = 2; else return -1;
    *is_profile = eat(p, "_profile");
    if (*is_profile && v == 2) return -1;
    int w;
    if (!strcmp(p, "_sat")) w = 0; else if (!strcmp(p, "_8")) w = 1; else if (!strcmp(p, "_16")) w = 2;
    else if (!strcmp(p, "_32")) w = 3; else if (!strcmp(p, "_64")) w = 4; else return -1;
    return ((m * N_OUT + o) * N_VEC + v) * N_WIDTH + w;
}

// ---- profiles --------------------------------------------------------------------------
struct parasail_profile {
    char *s1; int s1Len;
    const parasail_matrix_t *matrix;
    int stats; int width;
    // device copies of the query for the batch entries: one per device, uploaded on first use there, freed with the profile
    // (a Profile is Send + Sync in the reference, src/profile/mod.rs:392-395: threads driving different GPUs may share one)
    mutable std::vector<std::pair<int, uint8_t *>> *d_copies; mutable std::mutex *mx;
};

static parasail_profile_t *profile_new(const char *s1, int s1Len, const parasail_matrix_t *matrix, int stats, int width)
{
    if (!s1 || s1Len <= 0 || !matrix) return nullptr;       // -> Error::NullProfile (src/profile/mod.rs:101-103)
    parasail_profile_t *p = (parasail_profile_t *)calloc(1, sizeof *p);
    if (!p) return nullptr;
    p->s1 = (char *)malloc((size_t)s1Len + 1);
    if (!p->s1) { free(p); return nullptr; }
    memcpy(p->s1, s1, (size_t)s1Len); p->s1[s1Len] = 0;
    p->s1Len = s1Len; p->matrix = matrix; p->stats = stats; p->width = width;
    p->d_copies = new std::vector<std::pair<int, uint8_t *>>; p->mx = new std::mutex;
    return p;
}
extern "C" void parasail_profile_free(parasail_profile_t *p)
{
    if (!p) return;
    int cur = 0; const bool have_dev = hipGetDevice(&cur) == hipSuccess;
    for (auto &c : *p->d_copies) { if (have_dev) (void)hipSetDevice(c.first); (void)hipFree(c.second); }
    if (have_dev && !p->d_copies->empty()) (void)hipSetDevice(cur);
    delete p->d_copies; delete p->mx;
    free(p->s1); free(p);
}
// the query maps to a column beyond the first four of the matrix alphabet somewhere (the perm-table kernel cannot express that)
static int profile_has_wildcard(const parasail_profile_t *p)
{
    for (int i = 0; i < p->s1Len; ++i)
        if (p->matrix->mapper[(unsigned char)p->s1[i]] >= 4) return 1;
    return 0;
}

static int profile_device_query(const parasail_profile_t *p, const uint8_t **out)
{
    int dev = 0; HIP_OR_RET(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(*p->mx);
    for (auto &c : *p->d_copies) if (c.first == dev) { *out = c.second; return 0; }
    uint8_t *d = nullptr;
    HIP_OR_RET(hipMalloc(&d, (size_t)p->s1Len + 16));
    hipError_t e = hipMemcpy(d, p->s1, (size_t)p->s1Len, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); set_err("hipMemcpy: %s", hipGetErrorString(e)); return -(int)e; }
    p->d_copies->emplace_back(dev, d);
    *out = d;
    return 0;
}

#define PMX_DEFINE_PROFILE_CREATORS(ISA)                                                                    \
    extern "C" parasail_profile_t *parasail_profile_create##ISA##_sat(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 0, 0); }  \
    extern "C" parasail_profile_t *parasail_profile_create##ISA##_8(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 0, 8); }    \
    extern "C" parasail_profile_t *parasail_profile_create##ISA##_16(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 0, 16); }  \
    extern "C" parasail_profile_t *parasail_profile_create##ISA##_32(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 0, 32); }  \
    extern "C" parasail_profile_t *parasail_profile_create##ISA##_64(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 0, 64); }  \
    extern "C" parasail_profile_t *parasail_profile_create_stats##ISA##_sat(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 1, 0); }  \
    extern "C" parasail_profile_t *parasail_profile_create_stats##ISA##_8(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 1, 8); }    \
    extern "C" parasail_profile_t *parasail_profile_create_stats##ISA##_16(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 1, 16); }  \
    extern "C" parasail_profile_t *parasail_profile_create_stats##ISA##_32(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 1, 32); }  \
    extern "C" parasail_profile_t *parasail_profile_create_stats##ISA##_64(const char *s, const int n, const parasail_matrix_t *m) { return profile_new(s, n, m, 1, 64); }
PMX_DEFINE_PROFILE_CREATORS()
PMX_DEFINE_PROFILE_CREATORS(_sse_128)
PMX_DEFINE_PROFILE_CREATORS(_avx_256)
PMX_DEFINE_PROFILE_CREATORS(_neon_128)
PMX_DEFINE_PROFILE_CREATORS(_altivec_128)

// ---- one trampoline per dispatch name (a C function pointer carries no closure) ----------
template <int ID>
static parasail_result_t *tramp_f(const char *s1, const int s1Len, const char *s2, const int s2Len,
                                  const int open, const int gap, const parasail_matrix_t *matrix)
{
    return run_single(spec_from_id(ID), s1, s1Len, s2, s2Len, open, gap, matrix);
}
template <int ID>
static parasail_result_t *tramp_p(const parasail_profile_t *profile, const char *s2, const int s2Len,
                                  const int open, const int gap)
{
    if (!profile) die("NULL profile passed to a profile alignment function", hipSuccess);
    return run_single(spec_from_id(ID), profile->s1, profile->s1Len, s2, s2Len, open, gap, profile->matrix);
}
template <size_t... Is>
static parasail_function_t *const *make_ftable(std::index_sequence<Is...>)
{
    static parasail_function_t *const t[] = {&tramp_f<(int)Is>...};
    return t;
}
template <size_t... Is>
static parasail_pfunction_t *const *make_ptable(std::index_sequence<Is...>)
{
    static parasail_pfunction_t *const t[] = {&tramp_p<(int)Is>...};
    return t;
}

// src/aligner/mod.rs:345: NULL -> build() panics "Parasail function: {}, not found." (:353-358)
extern "C" parasail_function_t *parasail_lookup_function(const char *funcname)
{
    bool prof = false;
    const int id = parse_name(funcname, &prof);
    if (id < 0 || prof) return nullptr;
    return make_ftable(std::make_index_sequence<N_IDS>{})[id];
}
// src/aligner/mod.rs:349
extern "C" parasail_pfunction_t *parasail_lookup_pfunction(const char *funcname)
{
    bool prof = false;
    const int id = parse_name(funcname, &prof);
    if (id < 0 || !prof) return nullptr;
    return make_ptable(std::make_index_sequence<N_IDS>{})[id];
}

extern "C" int pmx_align_batch_banded(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                      const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                      int32_t band, const int32_t *diag, pmx_record_t *out);
// src/aligner/mod.rs:470-481.  Cells with |i-j| > k are excluded.
extern "C" parasail_result_t *parasail_nw_banded(const char *s1, const int s1Len, const char *s2, const int s2Len,
                                                 const int open, const int gap, const int k,
                                                 const parasail_matrix_t *matrix)
{
    RunSpec sp; memset(&sp, 0, sizeof sp);
    sp.mode = PMX_MODE_NW; sp.band = k < 0 ? 0 : k; sp.width = 32; sp.vecflag = 0;
    if (s1 && s2 && s1Len > 0 && s2Len > 0 && matrix && matrix->type == PARASAIL_MATRIX_TYPE_SQUARE && sp.band <= 63 &&
        matrix->size <= PMX_MAX_FAST_MSIZE) {
        // the band-only kernel: O(qlen * k) cells, no length limit ("for aligning large sequences", src/aligner/mod.rs:454-456)
        parasail_result_t *res = (parasail_result_t *)calloc(1, sizeof(parasail_result_t));
        if (!res) die("calloc", hipSuccess);
        res->qlen = s1Len; res->rlen = s2Len;
        res->flag = F_NW | F_BANDED | F_BITS_32;
        pmx_config_t cfg; memset(&cfg, 0, sizeof cfg);
        cfg.mode = PMX_MODE_NW; cfg.open = open; cfg.extend = gap; cfg.width = 32; cfg.matrix = matrix;
        const int64_t qo[2] = {0, s1Len}, ro[2] = {0, s2Len};
        pmx_record_t rec;
        if (pmx_align_batch_banded(&cfg, nullptr, 1, (const uint8_t *)s1, qo, (const uint8_t *)s2, ro, sp.band, nullptr, &rec))
            die(g_err, hipSuccess);
        res->score = rec.score; res->end_query = rec.end_query; res->end_ref = rec.end_ref;
        return res;
    }
    return run_single(sp, s1, s1Len, s2, s2Len, open, gap, matrix);
}

// ================================================================ traceback / CIGAR =====
// Host-side O(qlen+rlen) walk over the trace table the GPU produced (the reference's
// counterpart also runs on the host inside libparasail: src/alignment/mod.rs:390-419).
// State INS (E: consumes a reference char) prints 'D', state DEL (F: consumes a query char)
// prints 'I'  -- SAM sense with query = s1, reference = s2.  [UNPINNED, see DESIGN.md]
static const char CIG_INS_STATE = PMX_CIGAR_LETTER_FOR_INS_STATE, CIG_DEL_STATE = PMX_CIGAR_LETTER_FOR_DEL_STATE;   // include/pmx_conventions.h

static std::string walk_ops(const parasail_result_t *res, const char *seqA, int lena, const char *seqB, int lenb,
                            const parasail_matrix_t *matrix, int *beg_query, int *beg_ref)
{
    std::string rev;
    int i = res->end_query, j = res->end_ref;
    const bool sw = res->flag & F_SW, sg = res->flag & F_SG;
    if (sg) {
        if (i + 1 == lena) for (int k = lenb - 1; k > j; --k) rev.push_back(CIG_INS_STATE);
        else if (j + 1 == lenb) for (int k = lena - 1; k > i; --k) rev.push_back(CIG_DEL_STATE);
    }
    int where = PARASAIL_DIAG;
    while (i >= 0 || j >= 0) {
        if (i < 0) { if (sw) break; rev.push_back(CIG_INS_STATE); --j; continue; }
        if (j < 0) { if (sw) break; rev.push_back(CIG_DEL_STATE); --i; continue; }
        const int t = res->trace[(size_t)i * lenb + j];
        if (where == PARASAIL_DIAG) {
            if (t & PARASAIL_DIAG) {
                const bool eq = matrix->mapper[(unsigned char)seqA[i]] == matrix->mapper[(unsigned char)seqB[j]];
                rev.push_back(eq ? '=' : 'X'); --i; --j;
            } else if (t & PARASAIL_INS) where = PARASAIL_INS;
            else if (t & PARASAIL_DEL) where = PARASAIL_DEL;
            else break;
        } else if (where == PARASAIL_INS) {
            rev.push_back(CIG_INS_STATE);
            if (t & PARASAIL_DIAG_E) where = PARASAIL_DIAG;
            --j;
        } else {
            rev.push_back(CIG_DEL_STATE);
            if (t & PARASAIL_DIAG_F) where = PARASAIL_DIAG;
            --i;
        }
    }
    *beg_query = i + 1; *beg_ref = j + 1;
    return std::string(rev.rbegin(), rev.rend());
}

static const char BAM_OPS[] = "MIDNSHP=X";
// The letters of the two gap states are not pinned by anything the reference holds (include/pmx_conventions.h).  The compiled
// default can be exchanged at run time, without a rebuild, by a caller who holds real parasail output that says otherwise:
// PMX_CIGAR_SWAP_ID=1 swaps I and D in everything handed out (packed ops of get_cigar / ssw, decoded text, batch CIGAR text).
int pmx_cigar_swapped()
{
    const char *v = pmx_env("PMX_CIGAR_SWAP_ID");
    return v && *v && strcmp(v, "0") != 0;
}

extern "C" parasail_cigar_t *parasail_result_get_cigar(parasail_result_t *result, const char *seqA, int lena,
                                                       const char *seqB, int lenb, const parasail_matrix_t *matrix)
{
    if (!result || !result->trace || !matrix || lena != result->qlen || lenb != result->rlen) return nullptr;
    parasail_cigar_t *c = (parasail_cigar_t *)calloc(1, sizeof *c);
    if (!c) return nullptr;
    const std::string ops = walk_ops(result, seqA, lena, seqB, lenb, matrix, &c->beg_query, &c->beg_ref);
    c->seq = (uint32_t *)malloc(sizeof(uint32_t) * (ops.size() + 1));
    if (!c->seq) { free(c); return nullptr; }
    size_t k = 0; int n = 0;
    const int swap = pmx_cigar_swapped();
    while (k < ops.size()) {
        size_t run = 1;
        while (k + run < ops.size() && ops[k + run] == ops[k]) ++run;
        uint32_t op = (uint32_t)(strchr(BAM_OPS, ops[k]) - BAM_OPS);
        if (swap && (op == 1u || op == 2u)) op ^= 3u;             // I (1) <-> D (2)
        c->seq[n++] = ((uint32_t)run << 4) | op;
        k += run;
    }
    c->len = n;
    return c;
}

// src/alignment/mod.rs:410: the returned string is adopted by Rust with CString::from_raw
// and must be a plain malloc block.
extern "C" char *parasail_cigar_decode(parasail_cigar_t *cigar)
{
    if (!cigar) return nullptr;
    std::string s;
    for (int k = 0; k < cigar->len; ++k) {
        s += std::to_string(cigar->seq[k] >> 4);
        s.push_back(BAM_OPS[cigar->seq[k] & 0xF]);
    }
    char *out = (char *)malloc(s.size() + 1);
    if (out) memcpy(out, s.c_str(), s.size() + 1);
    return out;
}
extern "C" void parasail_cigar_free(parasail_cigar_t *cigar) { if (cigar) { free(cigar->seq); free(cigar); } }

// src/alignment/mod.rs:356-376: the three strings are malloc blocks adopted by Rust.
extern "C" parasail_traceback_t *parasail_result_get_traceback(parasail_result_t *result, const char *seqA, int lena,
        const char *seqB, int lenb, const parasail_matrix_t *matrix, char match, char pos, char neg)
{
    if (!result || !result->trace || !matrix || lena != result->qlen || lenb != result->rlen) return nullptr;
    int bq = 0, br = 0;
    const std::string ops = walk_ops(result, seqA, lena, seqB, lenb, matrix, &bq, &br);
    const size_t n = ops.size();
    parasail_traceback_t *tb = (parasail_traceback_t *)calloc(1, sizeof *tb);
    if (!tb) return nullptr;
    tb->query = (char *)malloc(n + 1); tb->comp = (char *)malloc(n + 1); tb->ref = (char *)malloc(n + 1);
    if (!tb->query || !tb->comp || !tb->ref) { free(tb->query); free(tb->comp); free(tb->ref); free(tb); return nullptr; }
    int i = bq, j = br;
    for (size_t k = 0; k < n; ++k) {
        const char o = ops[k];
        if (o == '=' || o == 'X') {
            const int s = matrix->matrix[(size_t)matrix->size *
                              (matrix->type == PARASAIL_MATRIX_TYPE_PSSM ? i : matrix->mapper[(unsigned char)seqA[i]]) +
                              matrix->mapper[(unsigned char)seqB[j]]];
            tb->query[k] = seqA[i]; tb->ref[k] = seqB[j];
            tb->comp[k] = (o == '=') ? match : (s > 0 ? pos : neg);
            ++i; ++j;
        } else if (o == CIG_INS_STATE) { tb->query[k] = '-'; tb->ref[k] = seqB[j]; tb->comp[k] = ' '; ++j; }
        else { tb->query[k] = seqA[i]; tb->ref[k] = '-'; tb->comp[k] = ' '; ++i; }
    }
    tb->query[n] = tb->comp[n] = tb->ref[n] = 0;
    return tb;
}
extern "C" void parasail_traceback_free(parasail_traceback_t *tb)
{
    if (tb) { free(tb->query); free(tb->comp); free(tb->ref); free(tb); }
}

// src/alignment/mod.rs:310-344 (print_traceback): blocks of `width` columns, names padded to
// name_width, optional summary line.
extern "C" void parasail_traceback_generic(const char *seqA, int lena, const char *seqB, int lenb,
        const char *nameA, const char *nameB, const parasail_matrix_t *matrix, parasail_result_t *result,
        char match, char pos, char neg, int width, int name_width, int use_stats)
{
    parasail_traceback_t *tb = parasail_result_get_traceback(result, seqA, lena, seqB, lenb, matrix, match, pos, neg);
    if (!tb) { printf("(no traceback available)\n"); return; }
    const int n = (int)strlen(tb->query);
    if (width <= 0) width = 80;
    int bq = 0, br = 0;
    (void)walk_ops(result, seqA, lena, seqB, lenb, matrix, &bq, &br);
    int qi = bq, ri = br, nmatch = 0, ngap = 0, nmis = 0;
    for (int k = 0; k < n; k += width) {
        const int w = (n - k < width) ? n - k : width;
        int qadv = 0, radv = 0;
        for (int c = 0; c < w; ++c) {
            if (tb->query[k + c] != '-') ++qadv;
            if (tb->ref[k + c] != '-') ++radv;
            if (tb->query[k + c] == '-' || tb->ref[k + c] == '-') ++ngap;
            else if (tb->comp[k + c] == match) ++nmatch; else ++nmis;
        }
        printf("\n%*s %9d %.*s %9d\n", name_width, nameB ? nameB : "", ri + 1, w, tb->ref + k, ri + radv);
        printf("%*s %9s %.*s\n", name_width, "", "", w, tb->comp + k);
        printf("%*s %9d %.*s %9d\n", name_width, nameA ? nameA : "", qi + 1, w, tb->query + k, qi + qadv);
        qi += qadv; ri += radv;
    }
    if (use_stats) {
        printf("\nLength: %d\nIdentity:   %d/%d\nMismatches: %d/%d\nGaps:       %d/%d\nScore: %d\n",
               n, nmatch, n, nmis, n, ngap, n, result->score);
    }
    parasail_traceback_free(tb);
}

// ===================================================================== SSW emulation ====
// src/aligner/mod.rs:491-529, src/alignment/mod.rs:506-551: local alignment with begin and
// end coordinates and a packed CIGAR.  Runs sw+trace on the GPU, walks the trace on the host.
extern "C" parasail_result_ssw_t *parasail_ssw(const char *s1, const int s1Len, const char *s2, const int s2Len,
                                               const int open, const int gap, const parasail_matrix_t *matrix)
{
    parasail_result_ssw_t *out = (parasail_result_ssw_t *)calloc(1, sizeof *out);
    if (!out) die("calloc", hipSuccess);
    RunSpec sp; memset(&sp, 0, sizeof sp);
    sp.mode = PMX_MODE_SW; sp.band = -1; sp.width = 32; sp.trace = true;
    parasail_result_t *r = run_single(sp, s1, s1Len, s2, s2Len, open, gap, matrix);
    if (r->trace) {
        parasail_cigar_t *c = parasail_result_get_cigar(r, s1, s1Len, s2, s2Len, matrix);
        out->score1 = (uint16_t)(r->score > 65535 ? 65535 : (r->score < 0 ? 0 : r->score));
        out->ref_end1 = r->end_ref; out->read_end1 = r->end_query;
        if (c) {
            out->ref_begin1 = c->beg_ref; out->read_begin1 = c->beg_query;
            out->cigar = c->seq; out->cigarLen = c->len;
            free(c);                   // the seq array is now owned by the ssw result
        }
    }
    parasail_result_free(r);
    return out;
}
extern "C" parasail_profile_t *parasail_ssw_init(const char *s1, const int s1Len, const parasail_matrix_t *matrix,
                                                 const int8_t score_size)
{
    (void)score_size;
    return profile_new(s1, s1Len, matrix, 1, 0);
}
extern "C" void parasail_result_ssw_free(parasail_result_ssw_t *r) { if (r) { free(r->cigar); free(r); } }

// ============================================================================ batches ===
static int check_cfg(const pmx_config_t *cfg)
{
    if (!cfg || !cfg->matrix) { set_err("null config or matrix"); return -1; }
    if (cfg->mode < 0 || cfg->mode > 2) { set_err("bad mode %d", cfg->mode); return -1; }
    if (cfg->width != 0 && cfg->width != 8 && cfg->width != 16 && cfg->width != 32 && cfg->width != 64) {
        set_err("bad width %d", cfg->width); return -1;
    }
    if (cfg->open < 0 || cfg->extend < 0) { set_err("gap penalties are passed as positive numbers"); return -1; }
    return 0;
}

// A PSSM in a batch: every query has the PSSM's length (min_qlen .. max_qlen: the lengths the entry can see), and its rows alone
// fit the general kernel's LDS -- the general kernel is the fallback of every request the PSSM forms of the shared-profile kernels
// do not serve.  0 fine (or not a PSSM), -1 refused with a message.
static int pssm_batch_check(const parasail_matrix_t *m, int32_t min_qlen, int32_t max_qlen)
{
    if (m->type != PARASAIL_MATRIX_TYPE_PSSM) return 0;
    if (min_qlen != m->length || max_qlen != m->length) {
        set_err("PSSM length %d differs from the query length (%d..%d)", m->length, min_qlen, max_qlen); return -1;
    }
    if ((((size_t)m->length * m->size * 2 + 15) & ~(size_t)15) > 160 * 1024) {
        set_err("PSSM of %d rows x %d symbols does not fit the general kernel's LDS", m->length, m->size); return -1;
    }
    return 0;
}

static bool fast_sw_eligible(const pmx_config_t *cfg)
{
    // (width 8 included: for local alignment the saturation rule only needs the score, see PmxBatch::sat_above;
    //  a PSSM: pmx_launch_sw16 routes it into the PSSM form of the shared-profile kernel only)
    return cfg->mode == PMX_MODE_SW && (cfg->want & ~PMX_WANT_SORTED) == 0 &&
           (cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE || cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM);
}

extern "C" const char *pmx_kernel_for(const pmx_config_t *cfg, int32_t max_qlen, int32_t max_rlen)
{
    if (check_cfg(cfg)) return "invalid";
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {       // (score only: the PSSM forms of the shared-profile kernels, as batches run them)
        if ((cfg->want & ~PMX_WANT_SORTED) == 0 && cfg->mode == PMX_MODE_SW && cfg->matrix->size <= PMX_MAX_FAST_MSIZE &&
            max_qlen <= 2048 && max_rlen <= 60000)
            return "pmx_sw16q_kernel";
        if ((cfg->want & ~PMX_WANT_SORTED) == 0 && cfg->mode != PMX_MODE_SW && cfg->width != 8 && cfg->open >= cfg->extend &&
            max_qlen <= 2048 && cfg->matrix->size < PMX_MAX_FAST_MSIZE)
            return "pmx_nwsg16q_kernel";
        return "pmx_general_kernel";
    }
    if (fast_sw_eligible(cfg) && cfg->matrix->size <= PMX_MAX_FAST_MSIZE && max_qlen <= 2048 && max_rlen <= 60000)
        return "pmx_sw16_kernel";
    if ((cfg->mode == PMX_MODE_NW || cfg->mode == PMX_MODE_SG) && (cfg->want & ~PMX_WANT_SORTED) == 0 &&
        cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE && cfg->open >= cfg->extend && max_qlen <= 2048 &&
        cfg->matrix->size < PMX_MAX_FAST_MSIZE)
        return "pmx_nwsg16_kernel";
    if ((cfg->mode == PMX_MODE_NW || cfg->mode == PMX_MODE_SG) && (cfg->want & ~PMX_WANT_SORTED) == PMX_WANT_STATS && cfg->width != 8 &&
        cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE && cfg->open >= cfg->extend && cfg->extend >= 1 &&
        max_qlen <= 1024 && cfg->matrix->size < PMX_MAX_FAST_MSIZE)
        return "pmx_stats16_kernel";
    if ((cfg->want & ~PMX_WANT_SORTED) == 0 && cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE && cfg->matrix->size <= 64 &&
        (cfg->mode == PMX_MODE_SW || (cfg->width != 8 && cfg->width != 16)))
        return "pmx_long32_kernel";
    return "pmx_general_kernel";
}

// grow-only per-(thread,device) scratch for the general kernel's band boundary rows
struct Scratch { void *p = nullptr; size_t cap = 0; int dev = -1; };
enum { SCR_BOUND = 0, SCR_TRACE = 1, SCR_OPS = 2, SCR_SORT = 3, SCR_RETRY = 4,
       SCR_HQ = 5, SCR_HR = 6, SCR_HQO = 7, SCR_HRO = 8, SCR_HREC = 9, SCR_HST = 10,      // staging of the host-buffer batch entry
       SCR_CIG = 11,                                                                     // device CIGAR entry: counts, begins, text lengths, scan scratch
       SCR_HTEXT = 12, SCR_HTOFF = 13,                                                   // staging of the host CIGAR entry
       SCR_HQ2 = 14, SCR_HR2 = 15,                                                       // 2-bit packed input as it arrived
       SCR_LONG = 16,                                                                    // boundary granules + band candidates of pmx_long.hip
       SCR_SEL = 17,                                                                     // hit selection: state, histogram, block counts, sort buffers (pmx_select.hip)
       SCR_SRCH = 18, SCR_GREF = 19,                                                     // profile search: hit list / diagonals / lengths / offsets / begins; gathered references
       SCR_PAIRS = 20, SCR_PGEN = 21,                                                    // set batches: two sets of chunk buffers (pmx_pairs.hip); enumerated descriptors
       SCR_PUP = 22, SCR_PREC = 23, SCR_PST = 24,                                        // set batches, host entries: uploaded descriptors, records, statistics
       SCR_PSRCH = 25,                                                                   // set search: a chunk's records and statistics (ChunkAlign: with a chosen strand its slots' too), hit positions, counts, select scratch
       SCR_PHIT = 26,                                                                    // set search, host entry: a slice's hit columns (HitCols), counts, first bad pair
       SCR_PTOPK = 27,                                                                   // per-query top-K: a chunk's records and statistics (ChunkAlign), tile survivors, the rows' running state, scan scratch
       SCR_PTHIT = 28,                                                                   // per-query top-K, host entry: a slice's hit columns (HitCols) and row arrays, counts, first bad pair
       SCR_SWFS = 29,                                                                    // frameshift entries: the strips' boundary columns (pmx_swfs.hip)
       SCR_FSWIN = 30,                                                                   // windowed frameshift traceback: a chunk's first-pass records and strands, narrowed descriptors, shifts, lengths, the violation count
       SCR_SEED = 31,                                                                    // k-mer seeding: a slice's position slots, match buffers, cluster flags, cut, rocPRIM scratch (pmx_seed.hip)
       SCR_SEEDHIT = 32,                                                                 // k-mer seeding, host entry: counts, row offsets, the candidates' columns
       SCR_UNGAP = 33,                                                                   // ungapped filter: the list's records, sort keys, keep flags, rocPRIM scratch (pmx_ungap.hip)
       SCR_UNGAPHIT = 34,                                                                // ungapped filter, host entries: the uploaded list, the kept candidates' columns, counts
       SCR_SLOTS = 35 };
static thread_local Scratch g_scratch_pool[SCR_SLOTS];
static int scratch_reserve(size_t bytes, void **out, int slot = SCR_BOUND)
{
    Scratch &g_scratch = g_scratch_pool[slot];
    int dev = 0; HIP_OR_RET(hipGetDevice(&dev));
    if (g_scratch.dev != dev || g_scratch.cap < bytes) {
        if (g_scratch.p) {                                     // (a block of another device is released on that device)
            if (g_scratch.dev != dev) (void)hipSetDevice(g_scratch.dev);
            (void)hipFree(g_scratch.p);
            if (g_scratch.dev != dev) (void)hipSetDevice(dev);
        }
        g_scratch.p = nullptr; g_scratch.cap = 0; g_scratch.dev = dev;
        HIP_OR_RET(hipMalloc(&g_scratch.p, bytes ? bytes : 16));
        g_scratch.cap = bytes;
    }
    *out = g_scratch.p;
    return 0;
}

static thread_local const char *g_last_kernel = "";
extern "C" const char *pmx_last_kernel(void) { return g_last_kernel; }
// the packed traceback roads: the sweep as its launcher named it (kernel, decision form) + the walk the plan names
static const char *trace_road_name(const char *sweep, const PmxTracePlan &p, const DevMat &dm, bool stats)
{
    static thread_local char name[160];
    snprintf(name, sizeof name, "%s + %s%s", sweep, p.walk == PMX_TRACE_WALK16 ? "pmx_walk16_kernel" : dm.d.pssm ? "pmx_walkp_kernel<pssm>" : "pmx_walkp_kernel",
             stats ? "/stats" : "");
    return name;
}

// What every general-kernel batch shares: the n pairs, the matrix (a PSSM by query row), the gap model, the configured width, no band.
static PmxGeneralArgs general_args(const pmx_config_t *cfg, const DevMat &dm, int64_t n,
                                   const uint8_t *d_qbuf, const int64_t *d_qoff, int q_shared,
                                   const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen)
{
    PmxGeneralArgs a; memset(&a, 0, sizeof a);
    a.qbuf = d_qbuf; a.qoff = q_shared ? nullptr : d_qoff; a.shared_qlen = q_shared;
    a.rbuf = d_rbuf; a.roff = d_roff; a.n = n; a.max_rlen = max_rlen;
    a.scores = dm.d.scores; a.mapper = dm.d.mapper; a.msize = dm.d.msize; a.mat_rows = dm.d.rows; a.pssm = dm.d.pssm;
    a.mode = cfg->mode; a.sg_flags = cfg->sg_flags; a.open = cfg->open; a.ext = cfg->extend;
    a.band = -1; a.bits = cfg->width;
    return a;
}

// General kernel (one wave per pair) over the batch `t` describes.  Its scratch -- the boundary row between 64-row bands, 8 ints
// per reference column, and for references beyond the LDS a mapped copy in HBM -- only has to cover the pairs of one launch:
// chunks of ~2 GB (PMX_GENERAL_CHUNK_BYTES).  With t.index set (a re-run of listed pairs) a chunk is a stretch of the list and the
// outputs stay indexed by pair; otherwise a chunk is a stretch of the batch and every per-pair pointer moves with it.
// band >= 0: cells with |(j - i) - diag[pair]| > band are excluded (diag == nullptr: the main diagonal).
static int general_batch(const PmxGeneralArgs &t, bool want_stats, hipStream_t st, const char *what = "general kernel launch failed")
{
    const int64_t n = t.n;
    const size_t stride = (size_t)8 * t.max_rlen;
    const bool fits = pmx_general_lds_fits(t.mat_rows, t.msize, t.max_rlen);
    const size_t rs_stride = fits ? 0 : (((size_t)t.max_rlen + 8 + 15) & ~(size_t)15);
    const size_t per_pair = stride * sizeof(int32_t) + rs_stride;
    const char *cb = pmx_env("PMX_GENERAL_CHUNK_BYTES");
    int64_t chunk = (int64_t)((cb && atof(cb) > 0 ? atof(cb) : 2e9) / (double)per_pair);
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    void *bound = nullptr;
    if (scratch_reserve((size_t)chunk * per_pair, &bound)) return -1;
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        PmxGeneralArgs a = t;
        a.n = (n - c0 < chunk) ? n - c0 : chunk;
        if (a.index) a.index += c0;
        else {
            a.roff += c0; if (a.qoff) a.qoff += c0; if (a.diag) a.diag += c0;
            if (a.rec) a.rec += c0; if (a.stats) a.stats += c0; if (a.tab_off) a.tab_off += c0;
        }
        a.bound = (int32_t *)bound; a.bound_stride = (long long)stride;
        if (!fits) { a.rs_scratch = (uint8_t *)bound + (size_t)chunk * stride * sizeof(int32_t); a.rs_stride = (long long)rs_stride; }
        const int rc = pmx_launch_general(a, want_stats, st);
        if (rc) { set_err("%s (%d)", what, rc); return rc < 0 ? rc : -1; }
    }
    return 0;
}

// ---- statistics of the profile arm by traceback ------------------------------------------------------------
// matches / similar / length are properties of the one path the coupled statistics tables follow (same decisions, same
// tie-breaks as the traceback bits): the shared-profile sweep writes the packed 4-bit records (14.75 instructions per two
// cells against 34 for the kernel that carries nine statistics planes) and the walk counts along the path.  Chunks bound
// the trace scratch; the walk of chunk c runs beside the sweep of chunk c + 1 on a second stream.
struct TraceWs { hipStream_t walk = nullptr, aux = nullptr, aux2 = nullptr; hipEvent_t sweep_done[3] = {nullptr, nullptr, nullptr}, walk_done[3] = {nullptr, nullptr, nullptr}, start = nullptr; int dev = -1; };
static thread_local TraceWs g_tws;
static int trace_ws_init()
{
    int dev = 0; HIP_OR_RET(hipGetDevice(&dev));
    if (g_tws.dev == dev) return 0;
    if (g_tws.walk) {                                   // the thread moved to another device: release the old device's objects
        (void)hipStreamDestroy(g_tws.walk); (void)hipStreamDestroy(g_tws.aux); (void)hipStreamDestroy(g_tws.aux2); (void)hipEventDestroy(g_tws.start);
        for (int k = 0; k < 3; ++k) { (void)hipEventDestroy(g_tws.sweep_done[k]); (void)hipEventDestroy(g_tws.walk_done[k]); }
        g_tws = TraceWs();
    }
    // the walk gets the higher priority: its few, latency-bound workgroups slip in between the sweep's as those retire
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    HIP_OR_RET(hipStreamCreateWithPriority(&g_tws.walk, hipStreamNonBlocking, prio_hi));
    HIP_OR_RET(hipStreamCreateWithFlags(&g_tws.aux, hipStreamNonBlocking));
    HIP_OR_RET(hipStreamCreateWithFlags(&g_tws.aux2, hipStreamNonBlocking));
    HIP_OR_RET(hipEventCreateWithFlags(&g_tws.start, hipEventDisableTiming));
    for (int k = 0; k < 3; ++k) {
        HIP_OR_RET(hipEventCreateWithFlags(&g_tws.sweep_done[k], hipEventDisableTiming));
        HIP_OR_RET(hipEventCreateWithFlags(&g_tws.walk_done[k], hipEventDisableTiming));
    }
    g_tws.dev = dev;
    return 0;
}

// ---- chunks of a traceback batch: how large, and how their sweeps and walks overlap ----------------------------
// Bytes of trace one chunk may take: `ceiling`, at most `share` of the free HBM; the value of a switch (tests force small chunks)
// replaces both.  The callers hold the constants and the measurements behind them.
static double chunk_budget(double ceiling, double share, const char *forced /* pmx_env() of the caller's switch, or nullptr */)
{
    if (forced) return atof(forced);
    size_t fb = 0, tb = 0;
    return hipMemGetInfo(&fb, &tb) == hipSuccess && share * (double)fb < ceiling ? share * (double)fb : ceiling;
}
// Pairs per chunk: as many equal chunks as `trace_bytes` needs under `budget`, at least `min_chunks` (what the caller's overlap
// wants for a batch of this size), rounded up to whole groups of 64 pairs.
static int64_t chunk_pairs(int64_t n, double trace_bytes, double budget, int64_t min_chunks)
{
    int64_t nchunks = (int64_t)(trace_bytes / budget) + 1;
    if (nchunks < min_chunks) nchunks = min_chunks;
    const int64_t chunk = ((n + nchunks - 1) / nchunks + 63) / 64 * 64;
    return chunk > n ? n : chunk;
}

// Typed arrays carved out of one block, each starting on a 256-byte boundary (the block's base is one: hipMalloc; align: another
// power of two for a host block).  The same sequence of take() calls runs twice -- over no block for the size, then over the reserved
// block -- so size and layout cannot disagree.
struct Carver {
    unsigned char *base = nullptr; size_t used = 0, align = 256;
    template <typename T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + used) : nullptr;
        used = (used + count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
};
// layout(Carver &) takes what the caller needs; the block comes from the scratch slot.
template <typename Layout> static int scratch_carve(int slot, Layout layout)
{
    Carver size, c; layout(size);
    if (scratch_reserve(size.used, (void **)&c.base, slot)) return -1;
    layout(c);
    return 0;
}

// What the walks leave per pair for the CIGAR text -- run-length ops in the pair's slot, their count, the text's length -- and the
// tail every device CIGAR road ends in on the caller's stream: one scan of the lengths into text offsets, one render of the slots.
struct SlotText {
    uint32_t *ops = nullptr; int32_t *nops = nullptr, *textlen = nullptr; void *scan = nullptr; size_t scan_bytes = 0;
    int reserve_ops(size_t slots) { return scratch_reserve(slots * sizeof(uint32_t), (void **)&ops, SCR_OPS); }
    void carve(Carver &c, int64_t n, bool text = true /* false: statistics only, no scan */)
    {
        nops = c.take<int32_t>((size_t)n); textlen = c.take<int32_t>((size_t)n + 2);
        scan_bytes = text ? pmx_text_scan_scratch_bytes(n) : 0;
        scan = c.take<unsigned char>(scan_bytes);
    }
    // slot of pair k: slot_qoff[k] + d_roff[k] + k - ops_base.  local_off (n + 1 entries of scratch): the batch is a later chunk of a
    // longer text -- d_text_off[0] already holds the total of the chunks before it and stays, the offsets continue from it
    int render(const int64_t *slot_qoff, const int64_t *d_roff, long long ops_base, int64_t n,
               char *d_text, int64_t capacity, int64_t *d_text_off, hipStream_t st, int64_t *local_off = nullptr) const
    {
        int rc = pmx_launch_text_offsets(textlen, n, local_off ? local_off : d_text_off, scan, scan_bytes, st);
        if (!rc && local_off) rc = pmx_launch_text_rebase(local_off, n, d_text_off, st);
        if (rc) { set_err("text offset scan failed (%d)", rc); return rc; }
        rc = pmx_launch_cigar_render_slots(ops, slot_qoff, d_roff, ops_base, nops, d_text_off, d_text, capacity, n, st);
        if (rc) { set_err("cigar render launch failed (%d)", rc); return rc; }
        return 0;
    }
};

// One chunk of overlap_chunks: pairs [c0, c0 + n), the idx-th chunk; its sweep goes to `sweep` into trace buffer `buf`, its walk to
// `walk` behind sweep_done, and walk_done (null when everything runs back to back on one stream) frees the buffer for chunk idx + 2.
struct ChunkTurn { int64_t c0, n; int idx, buf; hipStream_t sweep, walk; hipEvent_t sweep_done, walk_done; };
// The walk stream waits for the sweep just launched / the walk just launched is what the buffer's next sweep waits for: for bodies
// that launch sweep and walk themselves (pmx_launch_trace16 does both from the events in PmxWalkSplit).
static int chunk_sweep_launched(const ChunkTurn &t)
{
    if (!t.walk_done) return 0;
    HIP_OR_RET(hipEventRecord(t.sweep_done, t.sweep));
    HIP_OR_RET(hipStreamWaitEvent(t.walk, t.sweep_done, 0));
    return 0;
}
static int chunk_walk_launched(const ChunkTurn &t)
{
    if (t.walk_done) HIP_OR_RET(hipEventRecord(t.walk_done, t.walk));
    return 0;
}
// [0, n) in chunks of `chunk` pairs, body(turn) once per chunk (non-zero ends the loop and is returned).  two: two trace buffers,
// sweeps of consecutive chunks alternating between the caller's stream and an internal one (a chunk is a few thousand equally long
// waves: the tail of one launch is backfilled by the next), the walk of chunk c on the high-priority walk stream beside the sweep of
// chunk c + 1, and `st` continues behind the last walk; otherwise one buffer and sweep and walk back to back on `st`.
// (trace_ws_init() first.)
template <typename Body> static int overlap_chunks(int64_t n, int64_t chunk, bool two, hipStream_t st, Body body)
{
    if (two) { HIP_OR_RET(hipEventRecord(g_tws.start, st)); HIP_OR_RET(hipStreamWaitEvent(g_tws.aux, g_tws.start, 0)); }
    int idx = 0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk, ++idx) {
        const int slot = idx & 1;
        const ChunkTurn t = {c0, (n - c0 < chunk) ? n - c0 : chunk, idx, two ? slot : 0, (two && slot) ? g_tws.aux : st, two ? g_tws.walk : st,
                             g_tws.sweep_done[slot], two ? g_tws.walk_done[slot] : nullptr};
        if (two && idx >= 2) HIP_OR_RET(hipStreamWaitEvent(t.sweep, g_tws.walk_done[slot], 0));     // this trace buffer's last walk is done
        const int rc = body(t);
        if (rc) return rc;
    }
    if (two) HIP_OR_RET(hipStreamWaitEvent(st, g_tws.walk_done[(idx - 1) & 1], 0));      // the walk stream is in order: the last walk covers all
    return 0;
}

// Per-pair packed traceback over a batch the plan takes, in chunks of `chunk` pairs overlapped as overlap_chunks describes: the
// sweep and its trace bytes are planned for one chunk, with two trace buffers and two sets of block flags, or one.
// Per pair the walk leaves either the path's statistics (stats) or run-length ops in implicit slots (ops / ops_base) with their
// count, begins and CIGAR text length.  g_last_kernel: the last chunk's sweep + the walk.
struct TraceOutputs { pmx_stats_t *stats; uint32_t *ops; long long ops_base; int32_t *nops, *beg, *textlen; };
static size_t trace_flag_stride(int64_t chunk) { return (size_t)chunk / 2 + 16; }    // ints of one set of per-block flags
static int trace_chunks(const pmx_config_t *cfg, const DevMat &dm, const PmxBatch &b, int64_t chunk, bool two, int *bflags,
                        pmx_record_t *d_out, const TraceOutputs &o, hipStream_t st, const char *what)
{
    PmxBatch bc = b; bc.n = chunk;
    PmxTracePlan plan;
    if (pmx_trace16_plan(bc, dm.d, cfg->mode, cfg->open, cfg->extend, &plan) != 0 || plan.walk != PMX_TRACE_WALKP) return 1;
    const size_t cbytes = (plan.trace_bytes + 255) & ~(size_t)255;
    uint32_t *tbuf = nullptr;
    if (scratch_reserve(cbytes * (two ? 2 : 1), (void **)&tbuf, SCR_TRACE)) return -1;
    const size_t fstride = trace_flag_stride(chunk);
    const char *sweep = "";
    const int rc = overlap_chunks(b.n, chunk, two, st, [&](const ChunkTurn &t) -> int {
        const int64_t c0 = t.c0;
        PmxBatch bk = b;
        bk.n = t.n;
        bk.qoff = b.qoff + c0; bk.roff = b.roff + c0;
        bk.blockflag = bflags + (size_t)(t.idx & 1) * fstride;
        PmxWalkSplit sp = {t.walk, t.sweep_done, t.walk_done, o.ops_base - c0, o.textlen ? o.textlen + c0 : nullptr};
        const int rc = pmx_launch_trace16(plan, bk, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, d_out + c0,
                                          (uint32_t *)((unsigned char *)tbuf + (size_t)t.buf * cbytes),
                                          o.ops, nullptr, o.nops ? o.nops + c0 : nullptr, o.beg ? o.beg + 2 * c0 : nullptr, t.sweep, &sweep,
                                          o.stats ? o.stats + c0 : nullptr, &sp);
        if (rc) { set_err("%s (%d)", what, rc); return rc < 0 ? rc : -1; }
        return 0;
    });
    if (rc == 0) g_last_kernel = trace_road_name(sweep, plan, dm, o.stats != nullptr);
    return rc;
}

// 0 done (asynchronously on st), 1 not eligible, <0 error
// Upload progress of the calling host entry (pmx_align_profile_batch): reference slices still travelling on a copy stream.  A
// device routine that works through the batch in chunks of its own waits, per chunk, only for the slices that chunk reads.
struct UploadHook { int K = 0; int64_t hi[8]; hipEvent_t ev[8]; int waited[2] = {0, 0}; std::atomic<int> recorded{0}; std::atomic<int> failed{0}; };
static thread_local UploadHook *g_upload = nullptr;
static int upload_wait(int64_t upto /* references [0, upto) are about to be read */, hipStream_t st, int which /* 0 / 1: the stream's own progress */)
{
    UploadHook *u = g_upload;
    if (!u) return 0;
    int &w = u->waited[which];
    while (w < u->K && (w == 0 || u->hi[w - 1] < upto)) {
        while (u->recorded.load(std::memory_order_acquire) <= w && !u->failed.load()) std::this_thread::yield();   // (the uploading thread records the events)
        if (u->failed.load()) { set_err("upload of the references failed"); return -1; }
        HIP_OR_RET(hipStreamWaitEvent(st, u->ev[w], 0));
        ++w;
    }
    return 0;
}

static int stats_by_trace_shared(const pmx_config_t *cfg, const DevMat &dm, const PmxBatch &b,
                                 pmx_record_t *d_out, pmx_stats_t *d_stats, hipStream_t st)
{
    if (pmx_env("PMX_NO_STATS_BY_TRACE")) return 1;
    PmxTracePlan plan;
    if (pmx_nwsgq_trace_plan(b, dm.d, cfg->mode, cfg->open, cfg->extend, &plan) != 0) return 1;
    if (trace_ws_init()) return -1;
    const long long NP = plan.pairs_per_wg;
    // (measured on cfg 3: 8 GB chunks 55.0 ms, 24 GB 53.1 ms, 40 GB 51.0 ms)
    const double chunk_bytes = chunk_budget(40e9, 0.2, pmx_env("PMX_STATS_CHUNK_BYTES"));
    const double per_pair = (double)plan.trace_bytes / (double)b.n;
    long long chunk = (long long)(chunk_bytes / per_pair) / NP * NP;
    if (chunk < NP) chunk = NP;
    bool by_rounds = false;
    if (chunk >= b.n) chunk = b.n;
    else {
        // Whole ROUNDS of resident workgroups per chunk: the waves of a sweep over equally long references all take the same time,
        // so a launch of N workgroups runs for ceil(N / resident) rounds -- cfg 3 in three equal chunks of 1 042 workgroups each
        // (512 resident) ran 5 + 3 rounds where 6.1 were needed: 45.2 -> 42.5 ms (the remainder chunk first instead of last: 42.8).
        // Otherwise (a round does not fit a chunk): equal shares.
        const long long round = pmx_env("PMX_STATS_EQUAL_CHUNKS") ? 0 : pmx_nwsgq_trace_round_pairs(plan, dm.d, cfg->mode, cfg->sg_flags);
        if (round > 0 && chunk >= round) {
            chunk = chunk / round * round; by_rounds = true;
            if (g_upload) chunk = round;                       // (host entry: the references arrive in slices -- a sweep starts as soon as ONE round's worth is up)
        }
        else {
            const long long nch = (b.n + chunk - 1) / chunk;
            chunk = ((b.n + nch - 1) / nch + NP - 1) / NP * NP;
        }
    }
    PmxBatch bc = b; bc.n = chunk;
    (void)pmx_nwsgq_trace_plan(bc, dm.d, cfg->mode, cfg->open, cfg->extend, &plan);     // (the same shape: the bytes of one chunk)
    const size_t cbytes = (plan.trace_bytes + 255) & ~(size_t)255;
    // (PMX_STATS_NO_OVERLAP: sweep and walk of every chunk back to back on the caller's stream, one trace buffer -- the form the
    //  serialised kernel traces under profiles/ are taken in: per-launch durations of overlapping launches cannot be added up)
    const bool two = chunk < b.n && !pmx_env("PMX_STATS_NO_OVERLAP");
    // The remainder after the whole rounds (a few long waves that would end the call with the chip nearly idle, after waiting for a trace
    // buffer to come free: 3.1 ms of a 38 ms cfg-3 step for 1.7 % of the pairs, measured) goes FIRST, on a stream and a trace buffer of
    // its own, beside the first big chunks.  Not through the host entry: there the last references are the last to arrive.
    long long rem_n = 0;
    if (by_rounds && two && !g_upload && b.n % chunk != 0 && !pmx_env("PMX_STATS_TAIL_LAST")) rem_n = b.n % chunk;
    size_t rbytes = 0;
    if (rem_n) {
        PmxBatch br = b; br.n = rem_n;
        PmxTracePlan pr = plan;
        (void)pmx_nwsgq_trace_plan(br, dm.d, cfg->mode, cfg->open, cfg->extend, &pr);
        rbytes = pr.trace_bytes;
        if (pmx_nwsgq_trace_plan(br, dm.d, cfg->mode, cfg->open, cfg->extend, &pr, 1) == 0 && pr.trace_bytes > rbytes) rbytes = pr.trace_bytes;
        rbytes = (rbytes + 255) & ~(size_t)255;
    }
    uint32_t *tbuf = nullptr;
    if (scratch_reserve(cbytes * (two ? 2 : 1) + rbytes, (void **)&tbuf, SCR_TRACE)) return -1;
    const PmxEnds ends = pmx_ends(cfg->mode, cfg->sg_flags);      // (nw or sg: the plan above takes no other mode)
    // one chunk: positions [t.c0, t.c0 + t.n) of the batch; sweep into the t.buf-th trace buffer (of tb_bytes), the walk behind it
    const char *sweep = "", *tail_sweep = "";                  // (the road's name is the whole chunks' sweep, not the short tail's)
    auto run_chunk = [&](const ChunkTurn &t, size_t tb_bytes, bool short_waves) -> int {
        const long long c0 = t.c0;
        uint32_t *tb = (uint32_t *)((unsigned char *)tbuf + (size_t)t.buf * cbytes);
        PmxBatch bk = b;
        bk.n = t.n;
        pmx_record_t *out_k = d_out; pmx_stats_t *st_k = d_stats;
        if (b.perm) bk.perm = b.perm + c0;                    // positions c0 .. of the processing order; records stay indexed by pair
        else { bk.roff = b.roff + c0; out_k = d_out + c0; st_k = d_stats + c0; }
        if (!b.perm && upload_wait(c0 + bk.n, t.sweep, t.sweep == st ? 0 : 1)) return -1;                  // (host entry: this chunk's references are up)
        // The remainder after the whole rounds is less than one round: it runs on the shape with half the rows per lane (<32,10> for
        // <16,20> / <16,19>) -- twice the waves, each half as long
        PmxTracePlan pk = plan, p2;
        if (short_waves && plan.R >= 19 && !pmx_env("PMX_STATS_NO_SHORT_TAIL") &&
            pmx_nwsgq_trace_plan(bk, dm.d, cfg->mode, cfg->open, cfg->extend, &p2, 1) == 0 && p2.trace_bytes <= tb_bytes) pk = p2;
        int rc = pmx_launch_nwsgq_trace(pk, bk, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, out_k, tb, t.sweep, short_waves ? &tail_sweep : &sweep);
        if (rc) { set_err("shared-profile traceback sweep failed (%d)", rc); return rc < 0 ? rc : -1; }
        if ((rc = chunk_sweep_launched(t)) != 0) return rc;
        rc = pmx_launch_walkp(pk.G, pk.R, bk, dm.d, cfg->mode, cfg->open, cfg->extend, pk.Tmax, pk.top_aligned, st_k, ends.row_pen, ends.col_pen,
                              tb, out_k, nullptr, nullptr, 0, nullptr, nullptr, nullptr, t.walk);
        if (rc) { set_err("statistics walk failed (%d)", rc); return rc < 0 ? rc : -1; }
        return chunk_walk_launched(t);
    };
    // (the final join covers the remainder too: its walk went to the walk stream first, and that stream is in order)
    const int rc = overlap_chunks(b.n - rem_n, chunk, two, st, [&](const ChunkTurn &t) -> int {
        if (rem_n && t.idx == 0) {                             // the remainder: a third stream, trace buffer and pair of events, ahead of the first chunk
            HIP_OR_RET(hipStreamWaitEvent(g_tws.aux2, g_tws.start, 0));
            const ChunkTurn rem = {b.n - rem_n, rem_n, 0, 2, g_tws.aux2, g_tws.walk, g_tws.sweep_done[2], g_tws.walk_done[2]};
            const int rr = run_chunk(rem, rbytes, true);
            if (rr) return rr;
        }
        return run_chunk(t, cbytes, by_rounds && two && t.n < chunk);
    });
    if (rc) return rc;
    g_last_kernel = trace_road_name(sweep, plan, dm, true);
    return 0;
}

// Statistics of per-pair batches = counts along the packed traceback path (the same decisions and tie-breaks as the coupled
// statistics tables).  The packed traceback sweep runs at more than twice the speed of the statistics kernel and the walk is cheap;
// the trace scratch is bounded by working in chunks (no host synchronisation).  (A few pairs: the one-pass statistics kernel has the
// lower latency.)  0 done (asynchronously on st), 1 not eligible, <0 error.
static int stats_by_trace_pairs(const pmx_config_t *cfg, const DevMat &dm, const PmxBatch &b,
                                pmx_record_t *d_out, pmx_stats_t *d_stats, hipStream_t st)
{
    if (b.q_shared || !(b.n >= 2048 || pmx_env("PMX_STATS_BY_TRACE")) || pmx_env("PMX_NO_STATS_BY_TRACE")) return 1;
    const int64_t n = b.n;
    PmxBatch bt = b; bt.perm = nullptr;
    PmxTracePlan plan;
    if (pmx_trace16_plan(bt, dm.d, cfg->mode, cfg->open, cfg->extend, &plan) != 0 || plan.walk != PMX_TRACE_WALKP) return 1;
    const double budget = chunk_budget(8e9, 0.15, nullptr);
    const double per_pair = (double)plan.trace_bytes / (double)n + 1.0;
    int64_t nchunks = (int64_t)((double)plan.trace_bytes / budget) + 1;
    if (nchunks < 2 && n >= 16384) nchunks = 2;            // two chunks at least: the walk of one runs beside the sweep of the next
    int64_t chunk = ((n + nchunks - 1) / nchunks + 63) / 64 * 64;
    if ((double)chunk * per_pair > budget) chunk = (int64_t)(budget / per_pair) / 64 * 64;
    if (chunk < 64) chunk = 64;
    if (chunk > n) chunk = n;
    const bool two = chunk < n;
    if (two && trace_ws_init()) return -1;
    int *bflags = nullptr;
    if (scratch_reserve(2 * trace_flag_stride(chunk) * sizeof(int), (void **)&bflags, SCR_RETRY)) return -1;
    const TraceOutputs o = {d_stats, nullptr, 0, nullptr, nullptr, nullptr};
    return trace_chunks(cfg, dm, bt, chunk, two, bflags, d_out, o, st, "stats-by-traceback launch failed");
}

// The long-pair sweep's switches and scratch budget as both of its roads read them (long_batch, long_cigar_device); which form runs
// without a switch is each road's own decision, and what the form's scratch looks like is the planner's (pmx_long_plan).
static const size_t LONG_BUDGET_CEILING = ((size_t)4 << 30) + ((size_t)64 << 20);      // the most scratch one chunk of pairs takes
struct LongKnobs {
    bool two_columns = false, one_column = false;      // PMX_LONG_TWO_COLUMNS / PMX_LONG_ONE_COLUMN: force the form
    int rows_per_lane = 0;                 // PMX_LONG_ROWS_PER_LANE: 2, 4 or 16 (0: not set)
    // the bands of a pair wait for one another across workgroups; the wait is bounded (pmx_long.hip): ~2 us a poll
    int spin_limit = 1 << 20, chunk_cols = 16;
    size_t budget = LONG_BUDGET_CEILING; bool budget_forced = false;     // bytes of scratch one chunk may take (PMX_LONG_CHUNK_BYTES: tests force several chunks)
};
// The switches alone (no device needed) ...
static LongKnobs long_env_knobs()
{
    LongKnobs k;
    k.two_columns = pmx_env("PMX_LONG_TWO_COLUMNS") != nullptr; k.one_column = pmx_env("PMX_LONG_ONE_COLUMN") != nullptr;
    if (const char *e = pmx_env("PMX_LONG_ROWS_PER_LANE")) k.rows_per_lane = atoi(e) == 2 ? 2 : atoi(e) == 16 ? 16 : 4;
    if (const char *e = pmx_env("PMX_LONG_SPIN_LIMIT")) k.spin_limit = atoi(e);             // tests force the give-up path
    if (const char *e = pmx_env("PMX_LONG_CHUNK_COLS")) k.chunk_cols = atoi(e) == 64 ? 64 : 16;
    const char *e = pmx_env("PMX_LONG_CHUNK_BYTES");
    if ((k.budget_forced = e != nullptr)) k.budget = (size_t)atof(e);
    return k;
}
// ... and with the budget a call really has: a quarter of the free device memory, up to the ceiling.
static LongKnobs long_knobs()
{
    LongKnobs k = long_env_knobs();
    size_t fb = 0, tb = 0;
    if (hipMemGetInfo(&fb, &tb) != hipSuccess) fb = 0;
    if (!k.budget_forced) k.budget = std::min<size_t>(LONG_BUDGET_CEILING, fb / 4 + ((size_t)64 << 20));
    return k;
}
// The switches on top of a road's own choice of form.  rows_too: the score road also lets PMX_LONG_ROWS_PER_LANE pick the rows per lane
// and goes back to 256-row bands under PMX_LONG_ONE_COLUMN; the checkpoint road has its rows from the caller's band_rows and does neither.
static void long_apply_switches(const LongKnobs &k, bool rows_too, int *R, int *cols)
{
    if (k.two_columns) *cols = 2;
    if (k.one_column) { *cols = 1; if (rows_too) *R = 4; }
    if (rows_too && k.rows_per_lane) *R = k.rows_per_lane;
}

// The score road's sweep for n pairs: 0 planned, 1 not eligible.
static int long_score_plan(int mode, int64_t n, int32_t max_qlen, int32_t max_rlen, int msize, const LongKnobs &knobs, PmxLongPlan *pl)
{
    // R = 4 (256-row bands) also for batches that fill the chip: 1 024-row bands (R = 16) share a step's fixed work among four
    // times the rows, but the longer dependent chain per step costs more (512 x 5 kbp^2: 5.0 ms against 6.5 ms, measured)
    int R = 4;
    // The form with two columns per step (pmx_long32_kernel_c2) has the shorter time per column, the one-column form the shorter
    // lag from band to band, and 128-row bands (R = 2) halve a step at twice the bands.  One call of a few pairs is a latency
    // problem: time = columns x (ns per column) + bands x (ns of lag per band), constants measured on MI355X per form
    // (profiles/r04/long_shapes.txt); a batch that fills the chip keeps the one-column form with 256-row bands (throughput, measured).
    int cols = 1;
    if (n <= 16) {
        const bool sw = mode == PMX_MODE_SW;
        const double nb4 = (max_qlen + 255) / 256, nb2 = (max_qlen + 127) / 128, columns = max_rlen;
        // (ns per column and ns per band, measured at the end of round 4: local alignment in the plain form, global / semi-global in the
        //  form with column skew and row offset -- profiles/r04/long_shapes.txt, long_single_forms.txt)
        const double t1 = columns * (sw ? 156 : 115) + nb4 * (sw ? 18400 : 15700);
        const double t24 = columns * (sw ? 111 : 78.6) + nb4 * (sw ? 32600 : 20100);
        const double t22 = columns * (sw ? 85 : 62.4) + nb2 * (sw ? 23100 : 16400);
        if (t22 < 0.95 * t1 && t22 <= t24) { cols = 2; R = 2; }          // (within 5 %: the first form)
        else if (t24 < 0.95 * t1) cols = 2;
    }
    long_apply_switches(knobs, true, &R, &cols);
    PmxLongWant w = {};
    w.n = n; w.max_qlen = max_qlen; w.max_rlen = max_rlen; w.msize = msize; w.R = R; w.cols = cols; w.chunk_cols = knobs.chunk_cols;
    w.budget = knobs.budget; w.refuse_above_budget = !knobs.budget_forced; w.r16_above_4g = true;
    return pmx_long_plan(w, pl);
}

// pmx_long32_kernel over a batch, in chunks of bounded scratch: 0 done, 1 not eligible, < 0 error.  Score and end positions, 32-bit
// lanes, any gap model (open < extend included), alphabets up to 64 letters, no limit on either length.  Widths: local -- any
// (saturation = a score beyond the width); global / semi-global -- sat, 32, 64, or a fixed width whose range the boundary row /
// column already leaves (one pair: its lengths are known here); a fixed width that needs the range of H tracked is not served.
static int long_batch(const pmx_config_t *cfg, const DevMat &dm, const PmxBatch &b0, int64_t n, int32_t max_qlen, int32_t max_rlen,
                      pmx_record_t *d_out, hipStream_t st)
{
    if (pmx_env("PMX_NO_LONG_KERNEL") || cfg->matrix->type != PARASAIL_MATRIX_TYPE_SQUARE) return 1;
    int force_sat = 0, sat_above = 2147483647;
    const int wmax = cfg->width == 8 ? 127 : cfg->width == 16 ? 32767 : 2147483647;
    if (cfg->mode == PMX_MODE_SW) sat_above = wmax;
    else if (cfg->width == 8 || cfg->width == 16) {
        const PmxEnds ends = pmx_ends(cfg->mode, cfg->sg_flags);
        const long long lo = std::min(ends.col_pen ? -((long long)cfg->open + (long long)(max_qlen - 1) * cfg->extend) : 0LL,
                                      ends.row_pen ? -((long long)cfg->open + (long long)(max_rlen - 1) * cfg->extend) : 0LL);
        if (n == 1 && lo < -(long long)wmax - 1) force_sat = 1; else return 1;     // (inside the range: the general kernel tracks min / max H)
    }
    const LongKnobs knobs = long_knobs();
    PmxLongPlan pl;
    if (long_score_plan(cfg->mode, n, max_qlen, max_rlen, dm.d.msize, knobs, &pl)) return 1;
    void *scr = nullptr;
    if (scratch_reserve(pl.total, &scr, SCR_LONG)) return 1;
    HIP_OR_RET(hipMemsetAsync((unsigned char *)scr + pl.off_abort, 0, pl.abort_bytes, st));
    for (int64_t c0 = 0; c0 < n; c0 += pl.pairs) {
        PmxBatch b = b0;
        b.perm = nullptr;                                  // (a processing order is a hint: records are indexed by pair)
        b.n = (n - c0 < pl.pairs) ? n - c0 : pl.pairs;
        if (!b.q_shared) b.qoff = b0.qoff + c0;
        b.roff = b0.roff + c0;
        const int rc = pmx_launch_long(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, pl, scr, d_out + c0, sat_above, force_sat, knobs.spin_limit, st);
        if (rc < 0) { set_err("long-pair kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        if (rc) return c0 == 0 ? 1 : (set_err("long-pair kernel refused a later chunk"), -1);
    }
    // did a band give up waiting?  (The one host synchronisation of this path; one-pair calls synchronise right after anyway.)
    // (into pinned memory: an asynchronous copy to pageable memory goes through the runtime's staging thread, and the synchronisation
    //  behind it was seen to take 20-30 ms in steps of 10 ms for a 5 ms batch)
    static thread_local int *pin_flag = nullptr;
    if (!pin_flag) HIP_OR_RET(hipHostMalloc((void **)&pin_flag, 64, hipHostMallocDefault));
    *pin_flag = 0;
    HIP_OR_RET(hipMemcpyAsync(pin_flag, (unsigned char *)scr + pl.off_abort, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    const int gave_up = *pin_flag;
    if (gave_up) {
        set_err("long-pair kernel: a band's bounded wait for the band above ran out (dispatch order assumption broken, or PMX_LONG_SPIN_LIMIT); "
                "the call was redone on the per-pair kernels");
        return 1;
    }
    g_last_kernel = pl.name;
    return 0;
}

// Overflow promotion after the fast local kernel (`sat`, 32, 64): pairs whose int16 lanes overflowed are re-run in the 32-bit
// general kernel.  Skipped without any synchronisation when no score can reach 32768.  0 done, < 0 error.
static int promote_overflowed(const pmx_config_t *cfg, const DevMat &dm, const PmxBatch &b, pmx_record_t *d_out, hipStream_t st)
{
    const long long bound_score = (long long)(b.max_qlen < b.max_rlen ? b.max_qlen : b.max_rlen) *
                                  (cfg->matrix->max > 0 ? cfg->matrix->max : 0);
    // (the max3 variant of the fast kernel is exact up to 29 696 - max score; beyond that it sets
    //  PMX_FLAG_RERUN and the pair is redone here whatever the requested width)
    if (bound_score <= 27000) return 0;
    const int mask = PMX_FLAG_RERUN | ((cfg->width == 16 || cfg->width == 8) ? 0 : PMX_FLAG_SATURATED);
    DevBuf<int64_t> list; DevBuf<int> cnt;
    if (list.try_alloc((size_t)b.n) || cnt.try_alloc(1)) { set_err("out of device memory (promotion list)"); return -2; }
    int rc = pmx_launch_collect_saturated(d_out, b.n, list.p, cnt.p, mask, st);
    if (rc) { set_err("collect kernel failed (%d)", rc); return rc; }
    int count = 0;
    HIP_OR_RET(hipMemcpyAsync(&count, cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    if (count == 0) return 0;
    PmxGeneralArgs a = general_args(cfg, dm, count, b.qbuf, b.qoff, b.q_shared, b.rbuf, b.roff, b.max_rlen);
    a.index = list.p; a.rec = d_out;
    a.bits = cfg->width == 16 ? 16 : cfg->width == 8 ? 8 : 32;
    rc = general_batch(a, false, st, "promotion launch failed");
    if (rc) return rc;
    HIP_OR_RET(hipStreamSynchronize(st));      // the list is released on return
    return 0;
}

// Device-resident batch.  q_shared > 0: every pair uses the one query d_qbuf[0..q_shared) (profile arm).
static int run_batch_device(const pmx_config_t *cfg, int64_t n,
                            const uint8_t *d_qbuf, const int64_t *d_qoff, int q_shared,
                            const uint8_t *d_rbuf, const int64_t *d_roff,
                            int32_t max_qlen, int32_t max_rlen,
                            pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream,
                            int q_shared_wild /* shared query: it holds a letter beyond the first four (or unknown) */)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (max_qlen <= 0 || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    if ((cfg->want & PMX_WANT_STATS) && !d_stats_out) { set_err("stats requested without a stats buffer"); return -1; }
    if (cfg->want & PMX_WANT_CIGAR) { set_err("use pmx_align_batch_cigar for CIGAR output"); return -1; }
    if (pssm_batch_check(cfg->matrix, max_qlen, max_qlen)) return -1;
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    hipStream_t st = (hipStream_t)stream;
    PmxBatch b = {d_qbuf, d_qoff, d_rbuf, d_roff, n, max_qlen, max_rlen, q_shared, nullptr, nullptr, nullptr, 0, 0};
    const int want = cfg->want & ~PMX_WANT_SORTED;
    // A PSSM's scores do not depend on the query letters: score-only per-pair batches run on the PSSM forms of the shared-profile
    // kernels exactly as a profile batch does (b.q_shared = the PSSM's length; those forms read no query byte, no wildcard handling)
    if (dm.d.pssm && want == 0) { b.q_shared = max_qlen; q_shared_wild = 0; }
    if ((cfg->want & PMX_WANT_SORTED) && n >= 64 && n < (1LL << 32)) {
        void *scr = nullptr;
        if (scratch_reserve(pmx_sort_scratch_bytes(n), &scr, SCR_SORT)) return -1;
        const int rc = pmx_build_length_perm(d_roff, n, scr, &b.perm, st);
        if (rc < 0) { set_err("length sort failed (%d)", rc); return rc; }
    }
    // Few long pairs (one align() call on kilobases: src/aligner/mod.rs:397-430 has no length limit), or queries beyond the packed
    // kernels' 2 048 rows in any number: the query's bands spread over the chip (pmx_long.hip).
    long long long_min_cells = 250000;                     // (600 x 600: 0.18 ms here, 0.23-0.27 ms in the one-wave packed kernels)
    if (const char *e = pmx_env("PMX_LONG_MIN_CELLS")) long_min_cells = atoll(e);
    if (want == 0 && ((n <= 16 && max_qlen >= 512 && (long long)max_qlen * max_rlen >= long_min_cells) || max_qlen > 2048)) {
        const int rc = long_batch(cfg, dm, b, n, max_qlen, max_rlen, d_out, st);
        if (rc <= 0) return rc;
    }
    if (fast_sw_eligible(cfg)) {
        b.q_has_wildcard = b.q_shared ? q_shared_wild : 0;
        b.sat_above = cfg->width == 8 ? 127 : 0;
        if (n >= 4096 && n < (1LL << 32) && !b.q_has_wildcard) {
            // scratch that lets the launcher pick a kernel which hands some pairs back for a second launch
            void *scr = nullptr;
            if (scratch_reserve(((size_t)n + 1) * sizeof(unsigned), &scr, SCR_RETRY)) return -1;
            b.retry_count = (int *)scr;
            b.retry_list = (unsigned *)scr + 1;
        }
        const int rc = pmx_launch_sw16(b, dm.d, cfg->open, cfg->extend, d_out, st, &g_last_kernel);
        if (rc < 0) { set_err("sw16 launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        if (rc == 0) return promote_overflowed(cfg, dm, b, d_out, st);
        // rc == 1: shape not covered by the fast kernel -> general kernel below
    }
    if (q_shared && want == PMX_WANT_STATS && cfg->width != 8 && (cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE || dm.d.pssm) &&
        (cfg->mode == PMX_MODE_NW || cfg->mode == PMX_MODE_SG) && (n >= 512 || pmx_env("PMX_STATS_BY_TRACE"))) {
        // profile arm with statistics (BASELINE config 3): traceback sweep + counting walk (a PSSM: the PSSM forms of both)
        const int rc = stats_by_trace_shared(cfg, dm, b, d_out, d_stats_out, st);
        if (rc <= 0) return rc;
    }
    if (upload_wait(INT64_MAX, st, 0)) return -1;             // (host entry with a sliced upload: every other path reads the whole batch)
    if (want == PMX_WANT_STATS && cfg->width != 8 && cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE) {
        // Statistics, each step 0 done / 1 not eligible (the next one is tried) / < 0 error: (a) small alphabets: counts along the
        // packed traceback; (b) the packed statistics kernel (two pairs per lane slot; shared profile, or per-pair over a large
        // alphabet; global / semi-global inside its exact window); (c) large alphabets with short references: traceback again
        // (measured: per-pair protein 285 x 285, sw 0.37 -> 1.03 TCUPS, nw 0.40 -> 0.89 with the matrix-lookup traceback kernels;
        // against 5-kaa references the staged references and per-pair profiles starve the 16-rows-per-lane traceback shapes and the
        // statistics kernel wins); (d) the unpacked statistics kernel.
        auto launched = [](int rc, const char *what) {
            if (rc < 0) set_err("%s launch failed: %s", what, hipGetErrorString((hipError_t)(-rc)));
            return rc;
        };
        int rc = dm.d.msize <= 8 ? stats_by_trace_pairs(cfg, dm, b, d_out, d_stats_out, st) : 1;
        if (rc == 1)
            rc = launched(pmx_launch_stats16p(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, d_out, d_stats_out, st, &g_last_kernel), "stats16p");
        if (rc == 1 && dm.d.msize > 8 && (max_rlen <= 1024 || pmx_env("PMX_STATS_BY_TRACE_ANY")))
            rc = stats_by_trace_pairs(cfg, dm, b, d_out, d_stats_out, st);
        if (rc == 1)
            rc = launched(pmx_launch_stats16(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, d_out, d_stats_out, st, &g_last_kernel), "stats16");
        if (rc <= 0) return rc;
    }
    if ((cfg->mode == PMX_MODE_NW || cfg->mode == PMX_MODE_SG) && want == 0 && (cfg->width != 8 || !pmx_env("PMX_NWSG8_GENERAL")) &&
        (cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE || dm.d.pssm)) {
        // (width 8: the same int16 kernels, which then also track the range of H for the saturation flag -- the reference's
        //  narrowest width is its fastest on a CPU; it must not be the slow road here)
        b.track8 = cfg->width == 8;
        if (dm.d.msize <= 5 && n >= 2048 && !q_shared) {       // per-block flags: lets the launcher try the perm-table form first
            void *scr = nullptr;
            if (scratch_reserve(((size_t)n / 2 + 16) * sizeof(int), &scr, SCR_RETRY)) return -1;
            b.blockflag = (int *)scr;
        }
        const int rc = pmx_launch_nwsg16(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, d_out, st, &g_last_kernel);
        if (rc < 0) { set_err("nwsg16 launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        if (rc == 0) return 0;     // the host-side range proof makes overflow impossible: no promotion pass
    }
    if (want == 0) {
        // Outside every packed kernel's window (gap models with open < extend, alphabets of 32 and more letters, value ranges the
        // int16 lanes cannot prove): the 32-bit band kernel, one wave per 256 query rows -- several times the general kernel's rate
        const int rc = long_batch(cfg, dm, b, n, max_qlen, max_rlen, d_out, st);
        if (rc <= 0) return rc;
    }
    PmxGeneralArgs a = general_args(cfg, dm, n, d_qbuf, d_qoff, q_shared, d_rbuf, d_roff, max_rlen);
    a.max_qlen = max_qlen; a.rec = d_out; a.stats = d_stats_out;
    const int rcg = general_batch(a, (want & PMX_WANT_STATS) != 0, st);
    if (rcg) return rcg;
    g_last_kernel = dm.d.pssm ? "pmx_general_kernel/pssm" : "pmx_general_kernel";
    return 0;
}

// The device entries keep internal scratch (length-sort permutation, retry list, trace records, op slots) per HOST THREAD.  A thread
// that queues its next call on ANOTHER stream would let that call overwrite scratch the previous call's kernels may still read:
// every device entry therefore ends by recording an event on its stream, and a call that arrives on a different stream first makes
// its stream wait for that event.  Calls on one stream cost nothing extra; calls from different threads never share scratch.
struct StreamGuard {
    static thread_local hipEvent_t ev; static thread_local hipStream_t last; static thread_local int dev; static thread_local bool armed;
    hipStream_t st; bool ok;
    explicit StreamGuard(void *stream) : st((hipStream_t)stream), ok(true)
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) { ok = false; return; }
        if (dev != d) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; armed = false; dev = d; }
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ok = false; return; }
        if (armed && last != st && hipStreamWaitEvent(st, ev, 0) != hipSuccess) ok = false;
    }
    ~StreamGuard() { if (ok && ev && hipEventRecord(ev, st) == hipSuccess) { last = st; armed = true; } }
};
thread_local hipEvent_t StreamGuard::ev = nullptr;
thread_local hipStream_t StreamGuard::last = nullptr;
thread_local int StreamGuard::dev = -1;
thread_local bool StreamGuard::armed = false;

extern "C" int pmx_align_batch_device(const pmx_config_t *cfg, int64_t n,
                                      const uint8_t *d_qbuf, const int64_t *d_qoff,
                                      const uint8_t *d_rbuf, const int64_t *d_roff,
                                      int32_t max_qlen, int32_t max_rlen,
                                      pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream)
{
    if (check_cfg(cfg) || (n > 0 && pssm_batch_check(cfg->matrix, max_qlen, max_qlen))) return -1;     // (before any GPU work)
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return run_batch_device(cfg, n, d_qbuf, d_qoff, 0, d_rbuf, d_roff, max_qlen, max_rlen, d_out, d_stats_out, stream);
}

static void host_maxlens(int64_t n, const int64_t *off, int32_t *mx, bool *bad, int32_t *mn = nullptr)
{
    int64_t m = 0, lo = INT32_MAX;                  // (no stores inside the loop: one compare-select pair per element)
    for (int64_t k = 0; k < n; ++k) {
        const int64_t l = off[k + 1] - off[k];
        m = l > m ? l : m;
        lo = l < lo ? l : lo;
    }
    if (lo <= 0 || m > INT32_MAX) *bad = true;
    *mx = (int32_t)(m > INT32_MAX ? INT32_MAX : m);
    if (mn) *mn = (int32_t)(lo < 0 ? 0 : lo);
}
// A host batch staged on the device by plain synchronous copies: validated offsets and their maxima, references, queries (none with a
// profile: one shared query), optional per-pair diagonals, and room for the records.  For the entries whose device work dwarfs the
// transfer (banded, traced); host_batch, pmx_align_profile_batch and cigar_host_pipelined slice and pipeline theirs.
struct StagedBatch {
    DevBuf<uint8_t> dq, dr; DevBuf<int64_t> dqo, dro; DevBuf<int32_t> dd; DevBuf<pmx_record_t> drec;
    int64_t n = 0; int32_t mq = 0, mr = 0;
    int upload(const parasail_profile_t *profile, int64_t n_, const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
               const int32_t *diag)
    {
        n = n_;
        bool bad = false;
        host_maxlens(n, roff, &mr, &bad);
        if (!profile) host_maxlens(n, qoff, &mq, &bad); else mq = profile->s1Len;
        if (bad || roff[0] != 0 || (!profile && qoff[0] != 0)) { set_err("bad offsets (every sequence needs length >= 1, offsets start at 0)"); return -1; }
        if (dr.try_alloc((size_t)roff[n]) || dro.try_alloc(n + 1) || drec.try_alloc(n) || (diag && dd.try_alloc(n)) ||
            (!profile && (dq.try_alloc((size_t)qoff[n]) || dqo.try_alloc(n + 1)))) { set_err("out of device memory"); return -2; }
        HIP_OR_RET(hipMemcpy(dr.p, rbuf, (size_t)roff[n], hipMemcpyHostToDevice));
        HIP_OR_RET(hipMemcpy(dro.p, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
        if (diag) HIP_OR_RET(hipMemcpy(dd.p, diag, sizeof(int32_t) * n, hipMemcpyHostToDevice));
        if (!profile) {
            HIP_OR_RET(hipMemcpy(dq.p, qbuf, (size_t)qoff[n], hipMemcpyHostToDevice));
            HIP_OR_RET(hipMemcpy(dqo.p, qoff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
        }
        return 0;
    }
    int records(pmx_record_t *out) const { HIP_OR_RET(hipMemcpy(out, drec.p, sizeof(pmx_record_t) * n, hipMemcpyDeviceToHost)); return 0; }
};

// The same over both offset arrays of a large batch, split over a few host threads: the scan of 2 x 1M offsets is 1.2 ms on one
// core, as long as a third of the device work it precedes.
struct LenScan { int32_t mq = 0, mr = 0, mnr = INT32_MAX; bool bad = false; };
static LenScan scan_lengths(int64_t n, const int64_t *qoff, const int64_t *roff)
{
    const int T = n >= 262144 ? 4 : 1;
    LenScan part[4];
    auto work = [&](int t) {
        const int64_t a = n * t / T, e = n * (t + 1) / T;
        host_maxlens(e - a, qoff + a, &part[t].mq, &part[t].bad);
        host_maxlens(e - a, roff + a, &part[t].mr, &part[t].bad, &part[t].mnr);
    };
    // (thread creation can fail -- a process at its thread limit: std::system_error must not unwind through the C ABI; the
    //  parts without a helper are scanned here)
    std::thread th[3];
    bool started[3] = {false, false, false};
    for (int t = 1; t < T; ++t) {
        try { th[t - 1] = std::thread(work, t); started[t - 1] = true; } catch (const std::system_error &) {}
    }
    work(0);
    for (int t = 1; t < T; ++t) { if (started[t - 1]) th[t - 1].join(); else work(t); }
    LenScan r = part[0];
    for (int t = 1; t < T; ++t) {
        r.mq = std::max(r.mq, part[t].mq); r.mr = std::max(r.mr, part[t].mr); r.mnr = std::min(r.mnr, part[t].mnr); r.bad |= part[t].bad;
    }
    return r;
}
// ragged reference lengths: worth a length-sorted processing order
static pmx_config_t with_sort_hint(const pmx_config_t *cfg, int32_t min_rlen, int32_t max_rlen, int64_t n)
{
    pmx_config_t c = *cfg;
    if (n >= 256 && (long long)min_rlen * 5 < (long long)max_rlen * 4) c.want |= PMX_WANT_SORTED;
    return c;
}

// Streams and events of one host entry (one thread_local instance per entry): a copy stream, a compute stream, with `back` a third
// stream for the way back, and one upload / one finish event per slice.  Created on the thread's device, again after a move.
namespace {
struct HostStreams {
    hipStream_t copy = nullptr, comp = nullptr, back = nullptr; hipEvent_t up[8] = {}, done[8] = {}; int dev = -1;
    int init(bool with_back)
    {
        int d = 0; HIP_OR_RET(hipGetDevice(&d));
        if (dev == d) return 0;
        if (copy) {                                        // the thread moved to another device: release the old device's objects
            (void)hipStreamDestroy(copy); (void)hipStreamDestroy(comp); if (back) (void)hipStreamDestroy(back);
            for (int k = 0; k < 8; ++k) { (void)hipEventDestroy(up[k]); (void)hipEventDestroy(done[k]); }
            *this = HostStreams();
        }
        HIP_OR_RET(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        HIP_OR_RET(hipStreamCreateWithFlags(&comp, hipStreamNonBlocking));
        if (with_back) HIP_OR_RET(hipStreamCreateWithFlags(&back, hipStreamNonBlocking));
        for (int k = 0; k < 8; ++k) {
            HIP_OR_RET(hipEventCreateWithFlags(&up[k], hipEventDisableTiming));
            HIP_OR_RET(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
        }
        dev = d; return 0;
    }
};
}  // namespace

// Host buffers in, host records out.  packed2: the sequence buffers hold 2 bits per base (base b in byte b / 4 at bits 2 (b % 4),
// code c = letter c of the matrix alphabet) and the offsets count bases: a quarter of the bytes cross PCIe and a small kernel
// spells them out into the staging buffers before the slice is aligned.
static int host_batch(const pmx_config_t *cfg, int64_t n,
                      const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                      pmx_record_t *out, pmx_stats_t *stats_out, bool packed2)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (!qbuf || !qoff || !rbuf || !roff || !out) { set_err("null buffer"); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {           // (every query has the PSSM's length: checked before any GPU work)
        int32_t mq = 0, mnq = 0; bool bad = false;
        host_maxlens(n, qoff, &mq, &bad, &mnq);
        if (pssm_batch_check(cfg->matrix, mnq, mq)) return -1;
    }
    // the length scan runs beside the first transfers (it needs the host only; the offsets go up meanwhile)
    LenScan ls;
    std::future<void> scan;
    if (n >= 262144) {
        try { scan = std::async(std::launch::async, [&]() { ls = scan_lengths(n, qoff, roff); }); }
        catch (const std::system_error &) { ls = scan_lengths(n, qoff, roff); }          // no helper thread to be had: scan inline
    } else ls = scan_lengths(n, qoff, roff);
    struct ScanJoin { std::future<void> &f; ~ScanJoin() { if (f.valid()) f.wait(); } } scan_join{scan};     // (early returns)
    if (qoff[0] != 0 || roff[0] != 0) { set_err("offset arrays must start at 0"); return -1; }
    if (qoff[n] <= 0 || roff[n] <= 0 || qoff[n] > ((int64_t)1 << 40) || roff[n] > ((int64_t)1 << 40)) { set_err("bad offset arrays"); return -1; }
    const size_t qbytes = (size_t)qoff[n], rbytes = (size_t)roff[n];
    uint32_t letters = 0;
    if (packed2) {
        const char *al = cfg->matrix->alphabet;
        if (!al || strlen(al) < 4) { set_err("2-bit input needs a matrix alphabet of at least four letters"); return -1; }
        letters = (uint32_t)(unsigned char)al[0] | ((uint32_t)(unsigned char)al[1] << 8) | ((uint32_t)(unsigned char)al[2] << 16) | ((uint32_t)(unsigned char)al[3] << 24);
    }
    // device staging is kept per host thread between calls (hipMalloc / hipFree of hundreds of MB cost milliseconds)
    struct { uint8_t *p; } dq, dr, dq2 = {nullptr}, dr2 = {nullptr}; struct { int64_t *p; } dqo, dro; struct { pmx_record_t *p; } drec; struct { pmx_stats_t *p; } dst = {nullptr};
    const bool stats = cfg->want & PMX_WANT_STATS;
    if (stats && !stats_out) { set_err("stats requested without a stats buffer"); return -1; }
    if (scratch_reserve(qbytes + 16, (void **)&dq.p, SCR_HQ) || scratch_reserve(rbytes + 16, (void **)&dr.p, SCR_HR) ||
        scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dqo.p, SCR_HQO) || scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dro.p, SCR_HRO) ||
        scratch_reserve(sizeof(pmx_record_t) * n, (void **)&drec.p, SCR_HREC) ||
        (stats && scratch_reserve(sizeof(pmx_stats_t) * n, (void **)&dst.p, SCR_HST)) ||
        (packed2 && (scratch_reserve(qbytes / 4 + 16, (void **)&dq2.p, SCR_HQ2) || scratch_reserve(rbytes / 4 + 16, (void **)&dr2.p, SCR_HR2)))) return -1;
    static thread_local HostStreams hs;
    if (hs.init(true)) return -1;
    const hipStream_t s_copy = hs.copy, s_comp = hs.comp, s_back = hs.back; hipEvent_t *const s_ev = hs.up, *const s_done = hs.done;
    HIP_OR_RET(hipMemcpyAsync(dqo.p, qoff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    HIP_OR_RET(hipMemcpyAsync(dro.p, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    if (scan.valid()) scan.get();
    if (ls.bad) { (void)hipStreamSynchronize(s_copy); set_err("every sequence must have length >= 1"); return -1; }
    const int32_t mq = ls.mq, mr = ls.mr;
    const pmx_config_t cfg_s = with_sort_hint(cfg, ls.mnr, mr, n);
    cfg = &cfg_s;
    // Large uniform batches: the sequence bytes go up in slices on a copy stream while the previous slice is already being aligned
    // on a compute stream (the offsets are absolute, so a slice is just a pointer shift) and the slice before that travels back on a
    // third; over PCIe the transfer is several times the kernel time, this hides the kernel and the return trip behind it.
    const int K = (n >= 262144 && !(cfg->want & PMX_WANT_SORTED)) ? (packed2 ? 4 : 8) : 1;     // (2-bit input: the kernel, not the link, is the longer leg)
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = n * sl / K, e = n * (sl + 1) / K;
        if (e <= a) continue;
        if (packed2) {
            const int64_t qa = qoff[a] / 4, qe = (qoff[e] + 3) / 4, ra = roff[a] / 4, re = (roff[e] + 3) / 4;
            HIP_OR_RET(hipMemcpyAsync(dq2.p + qa, qbuf + qa, (size_t)(qe - qa), hipMemcpyHostToDevice, s_copy));
            HIP_OR_RET(hipMemcpyAsync(dr2.p + ra, rbuf + ra, (size_t)(re - ra), hipMemcpyHostToDevice, s_copy));
        } else {
            HIP_OR_RET(hipMemcpyAsync(dq.p + qoff[a], qbuf + qoff[a], (size_t)(qoff[e] - qoff[a]), hipMemcpyHostToDevice, s_copy));
            HIP_OR_RET(hipMemcpyAsync(dr.p + roff[a], rbuf + roff[a], (size_t)(roff[e] - roff[a]), hipMemcpyHostToDevice, s_copy));
        }
        HIP_OR_RET(hipEventRecord(s_ev[sl], s_copy));
        HIP_OR_RET(hipStreamWaitEvent(s_comp, s_ev[sl], 0));
        if (packed2) {
            int rc2 = pmx_launch_unpack2(dq2.p, dq.p, qoff[a], qoff[e], letters, s_comp);
            if (!rc2) rc2 = pmx_launch_unpack2(dr2.p, dr.p, roff[a], roff[e], letters, s_comp);
            if (rc2) { (void)hipStreamSynchronize(s_comp); set_err("2-bit unpack launch failed (%d)", rc2); return rc2; }
        }
        const int rc = pmx_align_batch_device(cfg, e - a, dq.p, dqo.p + a, dr.p, dro.p + a, mq, mr, drec.p + a,
                                              stats ? dst.p + a : nullptr, s_comp);
        if (rc) { (void)hipStreamSynchronize(s_comp); return rc; }
        HIP_OR_RET(hipEventRecord(s_done[sl], s_comp));
        }
    // the way back, slice by slice as they finish (a copy into pageable host memory blocks the host thread, so it is not issued
    // inside the loop above: the later slices are already queued and keep the GPU busy meanwhile)
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = n * sl / K, e = n * (sl + 1) / K;
        if (e <= a) continue;
        HIP_OR_RET(hipEventSynchronize(s_done[sl]));
            HIP_OR_RET(hipMemcpyAsync(out + a, drec.p + a, sizeof(pmx_record_t) * (size_t)(e - a), hipMemcpyDeviceToHost, s_back));
        if (stats) HIP_OR_RET(hipMemcpyAsync(stats_out + a, dst.p + a, sizeof(pmx_stats_t) * (size_t)(e - a), hipMemcpyDeviceToHost, s_back));
    }
    HIP_OR_RET(hipStreamSynchronize(s_back));
    return 0;
}

extern "C" int pmx_align_batch(const pmx_config_t *cfg, int64_t n,
                               const uint8_t *qbuf, const int64_t *qoff,
                               const uint8_t *rbuf, const int64_t *roff,
                               pmx_record_t *out, pmx_stats_t *stats_out)
{
    return host_batch(cfg, n, qbuf, qoff, rbuf, roff, out, stats_out, false);
}

extern "C" int pmx_align_batch_2bit(const pmx_config_t *cfg, int64_t n,
                                    const uint8_t *q2, const int64_t *qoff,
                                    const uint8_t *r2, const int64_t *roff,
                                    pmx_record_t *out, pmx_stats_t *stats_out)
{
    return host_batch(cfg, n, q2, qoff, r2, roff, out, stats_out, true);
}

extern "C" int pmx_align_profile_batch(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                       const uint8_t *rbuf, const int64_t *roff,
                                       pmx_record_t *out, pmx_stats_t *stats_out)
{
    if (check_cfg(cfg)) return -1;
    if (!profile) { set_err("null profile"); return -1; }
    if (n <= 0) return 0;
    if (!rbuf || !roff || !out) { set_err("null buffer"); return -1; }
    if (profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    if (pssm_batch_check(cfg->matrix, profile->s1Len, profile->s1Len)) return -1;
    int32_t mr = 0, mnr = 0; bool bad = false;
    host_maxlens(n, roff, &mr, &bad, &mnr);
    if (bad || roff[0] != 0) { set_err("bad reference offsets"); return -1; }
    const pmx_config_t cfg_s = with_sort_hint(cfg, mnr, mr, n);
    cfg = &cfg_s;
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    if (stats && !stats_out) { set_err("stats requested without a stats buffer"); return -1; }
    struct { const uint8_t *p; } dq;
    if (profile_device_query(profile, &dq.p)) return -1;
    // References go up in slices on a copy stream while the previous slice is aligned (a slice is sorted and aligned on its own:
    // the offsets are absolute, a slice is a pointer shift) and finished slices travel back; the device staging is kept per host
    // thread between calls.  cfg 5's eighth (3.4 GB of references) spends 60 ms on the link, all of it behind the kernels.
    const size_t rbytes = (size_t)roff[n];
    struct { uint8_t *p; } dr; struct { int64_t *p; } dro; struct { pmx_record_t *p; } drec; struct { pmx_stats_t *p; } dst = {nullptr};
    if (scratch_reserve(rbytes + 16, (void **)&dr.p, SCR_HR) || scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dro.p, SCR_HRO) ||
        scratch_reserve(sizeof(pmx_record_t) * n, (void **)&drec.p, SCR_HREC) ||
        (stats && scratch_reserve(sizeof(pmx_stats_t) * n, (void **)&dst.p, SCR_HST))) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t s_copy = hs.copy, s_comp = hs.comp; hipEvent_t *const s_up = hs.up, *const s_done = hs.done;
    const int dev = hs.dev;
    // (a slice must still fill the chip: at least 32 k references each)
    const int K = rbytes >= ((size_t)64 << 20) ? (int)std::max<int64_t>(1, std::min<int64_t>(8, n / 32768)) : 1;
    // slices of about equal bytes (the references may be ragged)
    int64_t lo[9]; lo[0] = 0; lo[K] = n;
    for (int sl = 1; sl < K; ++sl) {
        const int64_t target = (int64_t)(rbytes / K) * sl;
        lo[sl] = std::lower_bound(roff, roff + n + 1, target) - roff;
        if (lo[sl] < lo[sl - 1]) lo[sl] = lo[sl - 1];
        if (lo[sl] > n) lo[sl] = n;
    }
    HIP_OR_RET(hipMemcpyAsync(dro.p, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    const int wild = profile_has_wildcard(profile);
    if (stats && !(cfg->want & PMX_WANT_SORTED) && rbytes >= ((size_t)64 << 20)) {
        // Statistics of the profile arm are counted along a traceback that already works through the references in chunks of
        // its own (tens of thousands per launch, two launches in flight): cutting the batch into slices as below would shrink
        // those launches.  One call instead; the upload goes in eight slices and every chunk waits only for the slices it reads.
        UploadHook hook; hook.K = 8;
        for (int sl = 0; sl < 8; ++sl) { hook.hi[sl] = n * (sl + 1) / 8; hook.ev[sl] = s_up[sl]; }
        // (copies from pageable memory block the issuing thread: a helper issues them, this thread queues the kernels meanwhile)
        const hipStream_t copy_stream = s_copy;               // (thread-local objects of THIS thread: the helper gets them by value)
        uint8_t *const dr_base = dr.p;
        auto upload = [&hook, copy_stream, dr_base, dev, n, roff, rbuf]() {
            if (hipSetDevice(dev) != hipSuccess) { hook.failed.store(1); return; }
            for (int sl = 0; sl < 8; ++sl) {
                const int64_t a = n * sl / 8, e = n * (sl + 1) / 8;
                hipError_t er = e > a ? hipMemcpyAsync(dr_base + roff[a], rbuf + roff[a], (size_t)(roff[e] - roff[a]), hipMemcpyHostToDevice, copy_stream) : hipSuccess;
                if (er == hipSuccess) er = hipEventRecord(hook.ev[sl], copy_stream);
                if (er != hipSuccess) { hook.failed.store(1); return; }
                hook.recorded.store(sl + 1, std::memory_order_release);
            }
        };
        std::thread up;
        try { up = std::thread(upload); } catch (const std::system_error &) { upload(); }     // no helper: the copies are issued first
        g_upload = &hook;
        const int rc = run_batch_device(cfg, n, dq.p, nullptr, profile->s1Len, dr.p, dro.p, profile->s1Len, mr,
                                        drec.p, dst.p, s_comp, wild);
        g_upload = nullptr;
        if (up.joinable()) up.join();
        if (!rc && hook.failed.load()) { (void)hipStreamSynchronize(s_comp); set_err("upload of the references failed"); return -1; }
        if (rc) { (void)hipStreamSynchronize(s_comp); (void)hipStreamSynchronize(s_copy); return rc; }
        HIP_OR_RET(hipStreamSynchronize(s_comp));
        HIP_OR_RET(hipMemcpy(out, drec.p, sizeof(pmx_record_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_OR_RET(hipMemcpy(stats_out, dst.p, sizeof(pmx_stats_t) * (size_t)n, hipMemcpyDeviceToHost));
        return 0;
    }
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = lo[sl], e = lo[sl + 1];
        if (e <= a) continue;
        HIP_OR_RET(hipMemcpyAsync(dr.p + roff[a], rbuf + roff[a], (size_t)(roff[e] - roff[a]), hipMemcpyHostToDevice, s_copy));
        HIP_OR_RET(hipEventRecord(s_up[sl], s_copy));
        HIP_OR_RET(hipStreamWaitEvent(s_comp, s_up[sl], 0));
        const int rc = run_batch_device(cfg, e - a, dq.p, nullptr, profile->s1Len, dr.p, dro.p + a, profile->s1Len, mr,
                                        drec.p + a, stats ? dst.p + a : nullptr, s_comp, wild);
        if (rc) { (void)hipStreamSynchronize(s_comp); return rc; }
        HIP_OR_RET(hipEventRecord(s_done[sl], s_comp));
    }
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = lo[sl], e = lo[sl + 1];
        if (e <= a) continue;
        HIP_OR_RET(hipEventSynchronize(s_done[sl]));
        HIP_OR_RET(hipMemcpy(out + a, drec.p + a, sizeof(pmx_record_t) * (size_t)(e - a), hipMemcpyDeviceToHost));
        if (stats) HIP_OR_RET(hipMemcpy(stats_out + a, dst.p + a, sizeof(pmx_stats_t) * (size_t)(e - a), hipMemcpyDeviceToHost));
    }
    return 0;
}

// Device-resident references against one reused query profile, asynchronous on `stream`.
extern "C" int pmx_align_profile_batch_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                              const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen,
                                              pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream)
{
    if (check_cfg(cfg)) return -1;
    if (!profile) { set_err("null profile"); return -1; }
    if (profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    if (pssm_batch_check(cfg->matrix, profile->s1Len, profile->s1Len)) return -1;
    const uint8_t *dq = nullptr;
    if (profile_device_query(profile, &dq)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return run_batch_device(cfg, n, dq, nullptr, profile->s1Len, d_rbuf, d_roff, profile->s1Len, max_rlen,
                            d_out, d_stats_out, stream, profile_has_wildcard(profile));
}


// ---- banded batches (extension) ------------------------------------------------------------------------------
// The reference has one banded entry, Aligner::banded_nw -> parasail_nw_banded (src/aligner/mod.rs:454-489: global, main
// diagonal).  The batch form takes any mode and an optional per-pair band centre: cell (i, j) belongs to the band iff
// |(j - i) - diag[pair]| <= band.  BASELINE config 5's "banded SW" is this with mode = local and diag = end_ref - end_query of a
// first full pass (or a seed's diagonal).  Rule and oracle: oracle/pmx_oracle.c:orc_align_ex.
static int banded_device(const pmx_config_t *cfg, int64_t n, const uint8_t *d_qbuf, const int64_t *d_qoff, int q_shared,
                         const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_qlen, int32_t max_rlen,
                         int32_t band, const int32_t *d_diag, pmx_record_t *d_out, void *stream)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (band < 0) { set_err("band must be >= 0"); return -1; }
    if (max_qlen <= 0 || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    if (cfg->want & ~PMX_WANT_SORTED) { set_err("banded batches return score and end positions only"); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) { set_err("PSSM matrices are not supported by banded batches"); return -1; }
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    pmx_config_t c = *cfg; c.width = 32;                       // 32-bit lanes: no saturation inside a band
    const char *kname = "pmx_banded_kernel";
    void *sort_scr = nullptr, *retry_scr = nullptr;
    if (n >= 4096 && n < (1LL << 32) && scratch_reserve(pmx_sort_scratch_bytes(n), &sort_scr, SCR_SORT)) return -1;
    if (n < (1LL << 31) && scratch_reserve(2 * ((size_t)n + 1) * sizeof(unsigned), &retry_scr, SCR_RETRY)) return -1;      // two lists: wildcards, ties
    const int rcb = pmx_launch_banded(c.mode, c.sg_flags, c.open, c.extend, dm.d, n, d_qbuf, d_qoff, q_shared, d_rbuf, d_roff,
                                      max_qlen, max_rlen, band, d_diag, d_out, (hipStream_t)stream, &kname, sort_scr,
                                      retry_scr ? (unsigned *)retry_scr + 1 : nullptr, (int *)retry_scr);
    if (rcb < 0) { set_err("banded kernel launch failed: %s", hipGetErrorString((hipError_t)(-rcb))); return rcb; }
    if (rcb == 0) { g_last_kernel = kname; return 0; }
    PmxGeneralArgs a = general_args(&c, dm, n, d_qbuf, d_qoff, q_shared, d_rbuf, d_roff, max_rlen);
    a.max_qlen = max_qlen; a.band = band; a.diag = d_diag; a.rec = d_out;
    const int rc = general_batch(a, false, (hipStream_t)stream);
    if (rc == 0) g_last_kernel = "pmx_general_kernel/banded";
    return rc;
}

extern "C" int pmx_align_batch_banded_device(const pmx_config_t *cfg, int64_t n,
                                             const uint8_t *d_qbuf, const int64_t *d_qoff,
                                             const uint8_t *d_rbuf, const int64_t *d_roff,
                                             int32_t max_qlen, int32_t max_rlen, int32_t band, const int32_t *d_diag,
                                             pmx_record_t *d_out, void *stream)
{
    if (!d_qbuf || !d_qoff || !d_rbuf || !d_roff || !d_out) { set_err("null buffer"); return -1; }
    return banded_device(cfg, n, d_qbuf, d_qoff, 0, d_rbuf, d_roff, max_qlen, max_rlen, band, d_diag, d_out, stream);
}

extern "C" int pmx_align_profile_batch_banded_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                                     const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen,
                                                     int32_t band, const int32_t *d_diag, pmx_record_t *d_out, void *stream)
{
    if (!profile) { set_err("null profile"); return -1; }
    if (!cfg || profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    if (!d_rbuf || !d_roff || !d_out) { set_err("null buffer"); return -1; }
    const uint8_t *dq = nullptr;
    if (profile_device_query(profile, &dq)) return -1;
    return banded_device(cfg, n, dq, nullptr, profile->s1Len, d_rbuf, d_roff, profile->s1Len, max_rlen, band, d_diag, d_out, stream);
}

// Host buffers in, host records out.  profile != NULL: the profile arm (qbuf / qoff are ignored).
extern "C" int pmx_align_batch_banded(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                      const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                      int32_t band, const int32_t *diag, pmx_record_t *out)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (!rbuf || !roff || !out || (!profile && (!qbuf || !qoff))) { set_err("null buffer"); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) { set_err("PSSM matrices are not supported by banded batches"); return -1; }
    StagedBatch s;
    int rc = s.upload(profile, n, qbuf, qoff, rbuf, roff, diag);
    if (rc) return rc;
    rc = profile ? pmx_align_profile_batch_banded_device(cfg, profile, n, s.dr.p, s.dro.p, s.mr, band, s.dd.p, s.drec.p, nullptr)
                 : pmx_align_batch_banded_device(cfg, n, s.dq.p, s.dqo.p, s.dr.p, s.dro.p, s.mq, s.mr, band, s.dd.p, s.drec.p, nullptr);
    return rc ? rc : s.records(out);
}

// ---- score tables for a batch (extension; the reference returns one table per call, src/alignment/mod.rs:123-192) ----------
// d_tab_off[k] = number of cells before pair k's [qlen][rlen] int32 table in d_score_table (n + 1 entries); d_score_row is packed
// like the references (roff), d_score_col like the queries (qoff); any of the three outputs may be NULL.
extern "C" int pmx_align_batch_table_device(const pmx_config_t *cfg, int64_t n,
                                            const uint8_t *d_qbuf, const int64_t *d_qoff,
                                            const uint8_t *d_rbuf, const int64_t *d_roff,
                                            int32_t max_qlen, int32_t max_rlen,
                                            const int64_t *d_tab_off, int32_t *d_score_table,
                                            int32_t *d_score_row, int32_t *d_score_col,
                                            pmx_record_t *d_out, void *stream)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (!d_qbuf || !d_qoff || !d_rbuf || !d_roff) { set_err("null buffer"); return -1; }
    if (d_score_table && !d_tab_off) { set_err("a score table needs d_tab_off"); return -1; }
    if (max_qlen <= 0 || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    if (cfg->want & ~PMX_WANT_SORTED) { set_err("table batches return score tables, rows / columns and records"); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) { set_err("PSSM matrices are not supported by table batches"); return -1; }
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    int rc = pmx_launch_table(cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, dm.d, n, d_qbuf, d_qoff, 0, d_rbuf, d_roff,
                              max_qlen, max_rlen, d_tab_off, d_score_table, d_score_row, d_score_col, d_out, st);
    if (rc < 0) { set_err("table kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
    if (rc == 0) { g_last_kernel = "pmx_table_kernel"; return 0; }
    // outside the row-by-row kernel's window (references beyond 1 024 symbols, open < extend, ...): the general kernel, in chunks
    DevBuf<pmx_record_t> tmp_rec;
    if (!d_out && tmp_rec.try_alloc((size_t)n)) { set_err("out of device memory"); return -2; }
    PmxGeneralArgs a = general_args(cfg, dm, n, d_qbuf, d_qoff, 0, d_rbuf, d_roff, max_rlen);
    a.bits = 32; a.rec = d_out ? d_out : tmp_rec.p;
    a.tab_off = d_tab_off; a.score_table = d_score_table; a.score_row = d_score_row; a.score_col = d_score_col;
    rc = general_batch(a, false, st);
    if (rc) return rc;
    if (!d_out) HIP_OR_RET(hipStreamSynchronize(st));
    g_last_kernel = "pmx_general_kernel/tables";
    return 0;
}

// ---- device-resident CIGAR entry ------------------------------------------------------------------------
// Sweep (packed 4-bit traceback to HBM scratch) and walk run in chunks on two streams: the walk of chunk c (latency-bound, one
// lane per pair) runs beside the sweep of chunk c + 1 (VALU-bound); the trace scratch is double-buffered.  The walk leaves
// run-length ops in per-pair slots and each pair's text length; one scan and one render finish the batch on the caller's stream.
// 0 done (asynchronously on `st`), 1 not eligible for the packed traceback sweeps, <0 error.
// The offset arrays are absolute into d_qbuf / d_rbuf; ops_base = qoff[0] + roff[0] (0 when the offsets start at 0).
// What a set batch adds to the road (pmx_align_pairs_ex_device runs it once per chunk of pairs): the chunk's validity bytes -- a bad
// pair gets its record, an empty text and begins -1 / -1 between the walk and the text scan --, the begins as an output, and the
// text continuing behind the chunks before it (d_text_off[0] holds their total; d_text / capacity are the whole batch's).
struct CigarChunkOf { const uint8_t *ok = nullptr; int32_t *beg = nullptr; bool continues = false; };
static void set_err_no_cigar_road()
{
    set_err("this configuration has no device-resident CIGAR path (width 8, PSSM, open < extend, a matrix whose score + open "
            "leaves a byte, or queries beyond 1023 symbols): use pmx_align_batch_cigar");
}
// The road's window, from the configuration and the maxima alone: true when cigar_device_run takes the batch.
static bool cigar_device_eligible(const pmx_config_t *cfg, const DevMat &dm, int64_t n, int32_t mq, int32_t mr)
{
    if (cfg->width == 8 || cfg->matrix->type != PARASAIL_MATRIX_TYPE_SQUARE) return false;
    const PmxBatch b = {nullptr, nullptr, nullptr, nullptr, n, mq, mr, 0, nullptr, nullptr, nullptr, 0, 0};
    PmxTracePlan plan;
    return pmx_trace16_plan(b, dm.d, cfg->mode, cfg->open, cfg->extend, &plan) == 0 && plan.walk == PMX_TRACE_WALKP;
}
static int cigar_device_run(const pmx_config_t *cfg, const DevMat &dm, int64_t n,
                            const uint8_t *d_qbuf, const int64_t *d_qoff, const uint8_t *d_rbuf, const int64_t *d_roff,
                            int32_t mq, int32_t mr, long long ops_base,
                            pmx_record_t *d_out, char *d_text, int64_t capacity, int64_t *d_text_off, hipStream_t st,
                            const CigarChunkOf &set = CigarChunkOf())
{
    if (cfg->width == 8 || cfg->matrix->type != PARASAIL_MATRIX_TYPE_SQUARE) return 1;
    PmxBatch b = {d_qbuf, d_qoff, d_rbuf, d_roff, n, mq, mr, 0, nullptr, nullptr, nullptr, 0, 0};
    PmxTracePlan plan;
    if (pmx_trace16_plan(b, dm.d, cfg->mode, cfg->open, cfg->extend, &plan) != 0 || plan.walk != PMX_TRACE_WALKP) return 1;
    if (trace_ws_init()) return -1;
    // chunks: at most ~12 GB of trace each (two buffers; measured on 1.25 M pairs of 250 x 250: 3 GB chunks 27.8 ms, 12 GB 26.2 ms --
    // fewer launch tails), at most 15 % of the free HBM each, at least two for the overlap once the batch is worth it
    const int64_t chunk = chunk_pairs(n, (double)plan.trace_bytes, chunk_budget(12e9, 0.15, pmx_env("PMX_CIGAR_CHUNK_BYTES")), n >= 16384 ? 2 : 1);
    const bool two = chunk < n && !pmx_env("PMX_CIGAR_NO_OVERLAP");     // (diagnostics: sweep and walk back to back on one stream)
    SlotText t; int32_t *beg = nullptr; int *bflags = nullptr; int64_t *local_off = nullptr;
    if (t.reserve_ops((size_t)n * ((size_t)mq + mr + 1)) ||
        scratch_carve(SCR_CIG, [&](Carver &c) {
            t.carve(c, n);
            beg = c.take<int32_t>(2 * (size_t)n);
            bflags = c.take<int>(2 * trace_flag_stride(chunk));
            if (set.ok) local_off = c.take<int64_t>((size_t)n + 1);      // (every chunk of a set batch: the largest comes first, no later chunk grows the block)
        })) return -1;
    if (!set.continues) local_off = nullptr;
    const TraceOutputs o = {nullptr, t.ops, ops_base, t.nops, set.beg ? set.beg : beg, t.textlen};
    int rc = trace_chunks(cfg, dm, b, chunk, two, bflags, d_out, o, st, "traceback launch failed");
    if (rc) return rc;
    if (set.ok && (rc = pmx_launch_pairs_fixup_cigar(set.ok, n, d_out, t.nops, t.textlen, set.beg, st)) != 0) {
        set_err("bad-pair fix-up launch failed (%d)", rc); return rc;
    }
    return t.render(d_qoff, d_roff, ops_base, n, d_text, capacity, d_text_off, st, local_off);
}

extern "C" int pmx_align_batch_cigar_device(const pmx_config_t *cfg, int64_t n,
                                            const uint8_t *d_qbuf, const int64_t *d_qoff,
                                            const uint8_t *d_rbuf, const int64_t *d_roff,
                                            int32_t max_qlen, int32_t max_rlen,
                                            pmx_record_t *d_out, char *d_cigar_text, int64_t cigar_capacity,
                                            int64_t *d_cigar_off, void *stream)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (!d_qbuf || !d_qoff || !d_rbuf || !d_roff || !d_out || !d_cigar_text || !d_cigar_off) { set_err("null buffer"); return -1; }
    if (max_qlen <= 0 || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const int rc = cigar_device_run(cfg, dm, n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen, 0, d_out,
                                    d_cigar_text, cigar_capacity, d_cigar_off, (hipStream_t)stream);
    if (rc == 1) set_err_no_cigar_road();
    return rc == 1 ? -1 : rc;
}

// The caller-owned CIGAR text: a malloc block that grows chunk by chunk; device text is copied straight into it.
// Large text blocks go back to a small pool when the caller releases them with pmx_free(), and the next batch call starts from
// one: a caller that aligns batch after batch writes into memory that is already paged in (first-touch faults of a fresh
// 100 MB block cost milliseconds), and the block usually has the right size at once.  At most two blocks, at most 1 GB.
struct TextPool {
    std::mutex mx;
    std::unordered_map<void *, size_t> live;      // blocks handed to callers (capacity)
    std::vector<std::pair<char *, size_t>> idle;  // blocks given back
    static constexpr size_t MIN_BLOCK = 1 << 20, MAX_IDLE_BYTES = (size_t)1 << 30;
    char *take(size_t *cap)
    {
        std::lock_guard<std::mutex> lk(mx);
        if (idle.empty()) return nullptr;
        size_t best = 0;
        for (size_t k = 1; k < idle.size(); ++k) if (idle[k].second > idle[best].second) best = k;
        char *p = idle[best].first; *cap = idle[best].second;
        idle.erase(idle.begin() + (long)best);
        return p;
    }
    void handed_out(void *p, size_t cap) { if (cap >= MIN_BLOCK) { std::lock_guard<std::mutex> lk(mx); live[p] = cap; } }
    bool give_back(void *p)                        // true: the pool keeps it
    {
        std::lock_guard<std::mutex> lk(mx);
        auto it = live.find(p);
        if (it == live.end()) return false;
        const size_t cap = it->second;
        live.erase(it);
        size_t held = 0;
        for (auto &b : idle) held += b.second;
        if (idle.size() >= 2 || held + cap > MAX_IDLE_BYTES) return false;
        idle.emplace_back((char *)p, cap);
        return true;
    }
};
static TextPool g_text_pool;

// The caller-owned CIGAR text: a malloc block that grows chunk by chunk; device text is copied straight into it.
struct TextBuf {
    char *p = nullptr; size_t len = 0, cap = 0;
    char *grow(size_t extra)       // room for `extra` more bytes (+ terminator); returns the write position or nullptr
    {
        if (!p && extra + 1 >= TextPool::MIN_BLOCK / 2) p = g_text_pool.take(&cap);
        if (len + extra + 1 > cap) {
            size_t ncap = cap ? cap * 2 : 4096;
            while (ncap < len + extra + 1) ncap *= 2;
            char *np = (char *)realloc(p, ncap);
            if (!np) return nullptr;
            p = np; cap = ncap;
        }
        return p + len;
    }
};

// Terminates the finished text, hands the block to the caller (who releases it with pmx_free) and tells the pool.
static int publish_text(TextBuf &text, char **cigar_buf)
{
    if (!text.grow(0)) { set_err("out of memory"); return -1; }
    text.p[text.len] = 0;
    *cigar_buf = text.p; g_text_pool.handed_out(text.p, text.cap);
    return 0;
}

// The text stage of a host entry whose device run renders CIGAR text: a device buffer sized by the entry's estimate, one more run at the
// exact size where the text did not fit, then the text into a block of the caller's.
struct HostText {
    DevBuf<char> text; DevBuf<int64_t> off; int64_t capacity = 0;
    // buffers for n texts of `estimate` bytes together; 0, or -2 with the error set
    int alloc(int64_t n, int64_t estimate)
    {
        capacity = estimate;
        if (off.try_alloc((size_t)n + 1) || text.try_alloc((size_t)capacity + 1)) { set_err("out of device memory"); return -2; }
        return 0;
    }
    // fn(d_text, capacity, d_off) is the device run (its error is the stage's); the n + 1 offsets come back into host_off behind it -- on
    // *stream, which is then synchronised, or with a blocking copy (stream NULL) -- and a text of more than `capacity` bytes runs again at
    // its size.  Without alloc -- an entry whose call wants no text -- fn runs once without buffers.
    template <typename Fn>
    int run(int64_t n, int64_t *host_off, const hipStream_t *stream, Fn fn)
    {
        for (int pass = 0; pass < 2; ++pass) {
            const int rc = fn(text.p, capacity, off.p);
            if (rc || !off.p) return rc;
            if (stream) {
                HIP_OR_RET(hipMemcpyAsync(host_off, off.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, *stream));
                HIP_OR_RET(hipStreamSynchronize(*stream));
            } else HIP_OR_RET(hipMemcpy(host_off, off.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
            if (host_off[n] <= capacity) break;
            capacity = host_off[n];                           // rare: the text did not fit the estimate -- again with the exact size
            (void)hipFree(text.p); text.p = nullptr;
            if (text.try_alloc((size_t)capacity + 1)) { set_err("out of device memory"); return -2; }
        }
        return 0;
    }
    hipError_t copy_to(char *dst, int64_t bytes) const { return bytes ? hipMemcpy(dst, text.p, (size_t)bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    // the finished text of `bytes` bytes as a block of the caller's (released with pmx_free)
    int to_block(int64_t bytes, char **cigar_buf) const
    {
        TextBuf t;
        char *dst = t.grow((size_t)bytes);
        if (!dst) { set_err("out of memory"); return -1; }
        const hipError_t e = copy_to(dst, bytes);
        if (e != hipSuccess) { free(t.p); set_err("%s", hipGetErrorString(e)); return -(int)e; }
        t.len = (size_t)bytes;
        return publish_text(t, cigar_buf);
    }
};

// CIGAR for a batch.  Fast path: pmx_trace16 (4-bit trace in HBM, on-device walk); otherwise the general
// kernel with byte trace tables and pmx_walk_kernel.  Only the run-length ops come back to the host, which
// renders the text.  One chunk = one set of launches; chunks bound the trace scratch.
// PMX_TIMING=1: stage times of the batch CIGAR entry on stderr
struct StageTimer {
    bool on; double t0; const char *what;
    static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
    StageTimer() : on(pmx_env("PMX_TIMING") != nullptr), t0(now()), what("") {}
    void done(const char *stage) { if (on) { (void)hipDeviceSynchronize(); const double t = now(); fprintf(stderr, "[pmx timing] %-28s %8.3f ms\n", stage, (t - t0) * 1e3); t0 = t; } }
};

static int cigar_chunk(const pmx_config_t *cfg, const DevMat &dm, int64_t n,
                       const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                       pmx_record_t *out, TextBuf &text, int64_t *cigar_off /* n+1, cigar_off[0] preset */)
{
    StageTimer tm;
    int32_t mq = 0, mr = 0; bool bad = false;
    host_maxlens(n, qoff, &mq, &bad); host_maxlens(n, roff, &mr, &bad);
    if (bad || qoff[0] != 0 || roff[0] != 0) { set_err("bad offsets"); return -1; }
    std::vector<int64_t> ops_off(n + 1);
    ops_off[0] = 0;
    for (int64_t k = 0; k < n; ++k) ops_off[k + 1] = ops_off[k] + (qoff[k + 1] - qoff[k]) + (roff[k + 1] - roff[k]) + 1;
    const size_t qbytes = (size_t)qoff[n], rbytes = (size_t)roff[n];
    DevBuf<uint8_t> dq, dr; DevBuf<int64_t> dqo, dro, doo; DevBuf<pmx_record_t> drec; DevBuf<int32_t> dnops, dbeg;
    if (dq.try_alloc(qbytes) || dr.try_alloc(rbytes) || dqo.try_alloc(n + 1) || dro.try_alloc(n + 1) || doo.try_alloc(n + 1) ||
        drec.try_alloc(n) || dnops.try_alloc(n) || dbeg.try_alloc(2 * n)) { set_err("out of device memory"); return -2; }
    uint32_t *dops = nullptr;
    if (scratch_reserve((size_t)ops_off[n] * sizeof(uint32_t), (void **)&dops, SCR_OPS)) return -1;
    tm.done("host prep + device alloc");
    HIP_OR_RET(hipMemcpy(dq.p, qbuf, qbytes, hipMemcpyHostToDevice));
    HIP_OR_RET(hipMemcpy(dr.p, rbuf, rbytes, hipMemcpyHostToDevice));
    HIP_OR_RET(hipMemcpy(dqo.p, qoff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
    HIP_OR_RET(hipMemcpy(dro.p, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
    HIP_OR_RET(hipMemcpy(doo.p, ops_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));

    tm.done("H2D");
    PmxBatch b = {dq.p, dqo.p, dr.p, dro.p, n, mq, mr, 0, nullptr, nullptr, nullptr, 0, 0};
    PmxTracePlan plan;
    int rc;
    if (cfg->width != 8 && cfg->matrix->type == PARASAIL_MATRIX_TYPE_SQUARE &&
        pmx_trace16_plan(b, dm.d, cfg->mode, cfg->open, cfg->extend, &plan, false) == 0) {   // (packed sweeps: the pipelined path)
        uint32_t *tbuf = nullptr;
        if (scratch_reserve(plan.trace_bytes, (void **)&tbuf, SCR_TRACE)) return -1;
        const char *sweep = "pmx_trace16_kernel";
        rc = pmx_launch_trace16(plan, b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, drec.p, tbuf,
                                dops, doo.p, dnops.p, dbeg.p, nullptr, &sweep);
        g_last_kernel = trace_road_name(sweep, plan, dm, false);
        if (rc) { set_err("trace16 launch failed (%d)", rc); return rc < 0 ? rc : -1; }
    } else {
        std::vector<int64_t> tab_off(n + 1);
        tab_off[0] = 0;
        for (int64_t k = 0; k < n; ++k) tab_off[k + 1] = tab_off[k] + (qoff[k + 1] - qoff[k]) * (roff[k + 1] - roff[k]);
        DevBuf<int64_t> dto;
        if (dto.try_alloc(n + 1)) { set_err("out of device memory"); return -2; }
        HIP_OR_RET(hipMemcpy(dto.p, tab_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
        int8_t *dtrace = nullptr;
        if (scratch_reserve((size_t)tab_off[n], (void **)&dtrace, SCR_TRACE)) {
            set_err("a byte trace table of %lld bytes could not be reserved; pmx_align_batch_cigar_long traces long pairs in linear memory", (long long)tab_off[n]);
            return -1;
        }
        PmxGeneralArgs a = general_args(cfg, dm, n, dq.p, dqo.p, 0, dr.p, dro.p, mr);
        a.rec = drec.p; a.tab_off = dto.p; a.trace_table = dtrace;
        rc = general_batch(a, false, nullptr);
        if (rc) return rc;
        PmxWalkArgs w; memset(&w, 0, sizeof w);
        w.qbuf = dq.p; w.qoff = dqo.p; w.rbuf = dr.p; w.roff = dro.p; w.n = n;
        w.mapper = dm.d.mapper; w.mode = cfg->mode; w.trace_table = dtrace; w.tab_off = dto.p; w.rec = drec.p;
        w.ops = dops; w.ops_off = doo.p; w.nops = dnops.p; w.beg = dbeg.p;
        rc = pmx_launch_walk(w, nullptr);
        g_last_kernel = "pmx_general_kernel + pmx_walk_kernel";
        if (rc) { set_err("walk kernel launch failed (%d)", rc); return rc < 0 ? rc : -1; }
        HIP_OR_RET(hipDeviceSynchronize());      // dto is released on scope exit
    }
    tm.done("sweep + walk kernels");
    // The CIGAR text is rendered on the device: text lengths come back (4 bytes per pair), the host turns them
    // into offsets, the text itself is written there and copied back in one piece.
    HIP_OR_RET(hipMemcpy(out, drec.p, sizeof(pmx_record_t) * n, hipMemcpyDeviceToHost));
    DevBuf<int32_t> dtl;
    if (dtl.try_alloc(n)) { set_err("out of device memory"); return -2; }
    rc = pmx_launch_cigar_textlen(dops, doo.p, dnops.p, dtl.p, n, nullptr);
    if (rc) { set_err("cigar length kernel launch failed (%d)", rc); return rc < 0 ? rc : -1; }
    std::vector<int32_t> tl(n);
    HIP_OR_RET(hipMemcpy(tl.data(), dtl.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    std::vector<int64_t> toff(n + 1);
    toff[0] = 0;
    for (int64_t k = 0; k < n; ++k) toff[k + 1] = toff[k] + tl[k];
    DevBuf<int64_t> dtoff; DevBuf<char> dtext;
    if (dtoff.try_alloc(n + 1) || dtext.try_alloc((size_t)toff[n] + 1)) { set_err("out of device memory"); return -2; }
    HIP_OR_RET(hipMemcpy(dtoff.p, toff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
    rc = pmx_launch_cigar_render(dops, doo.p, dnops.p, dtoff.p, dtext.p, n, nullptr);
    if (rc) { set_err("cigar render kernel launch failed (%d)", rc); return rc < 0 ? rc : -1; }
    const size_t base = text.len;
    char *dst = text.grow((size_t)toff[n]);
    if (!dst) { set_err("out of memory"); return -1; }
    if (toff[n]) HIP_OR_RET(hipMemcpy(dst, dtext.p, (size_t)toff[n], hipMemcpyDeviceToHost));
    text.len += (size_t)toff[n];
    for (int64_t k = 0; k < n; ++k) cigar_off[k + 1] = (int64_t)base + toff[k + 1];
    tm.done("render + D2H");
    return 0;
}

// Host entry on top of the device entry: the sequence bytes go up in slices on a copy stream, every slice runs the device
// pipeline (sweep / walk overlapped inside) on a compute stream as soon as its bytes have arrived, and the host copies a finished
// slice's records, offsets and text back while the following slices compute.  0 done, 1 not eligible, <0 error.
static int cigar_host_pipelined(const pmx_config_t *cfg, const DevMat &dm, int64_t n,
                                const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                pmx_record_t *out, TextBuf &text, int64_t *cigar_off)
{
    StageTimer tm;
    int32_t mq = 0, mr = 0; bool bad = false;
    host_maxlens(n, qoff, &mq, &bad); host_maxlens(n, roff, &mr, &bad);
    if (bad) { set_err("every sequence must have length >= 1"); return -1; }
    if (!cigar_device_eligible(cfg, dm, n, mq, mr)) return 1;          // before anything is staged
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t s_copy = hs.copy, s_comp = hs.comp; hipEvent_t *const s_up = hs.up, *const s_done = hs.done;
    const int K = n >= 262144 ? 8 : n >= 32768 ? 2 : 1;
    const size_t qbytes = (size_t)qoff[n], rbytes = (size_t)roff[n];
    // text capacity per slice: half a byte per sequence symbol + 16 per pair covers related reads many times over; a slice
    // that needs more is rendered again into an exact-size buffer (the ops are still in the scratch)
    int64_t cap[8], tbase[8], lo[8], hi[8];
    int64_t cap_total = 0;
    for (int sl = 0; sl < K; ++sl) {
        lo[sl] = n * sl / K; hi[sl] = n * (sl + 1) / K;
        cap[sl] = ((qoff[hi[sl]] - qoff[lo[sl]]) + (roff[hi[sl]] - roff[lo[sl]])) / 2 + 16 * (hi[sl] - lo[sl]) + 256;
        cap[sl] = (cap[sl] + 255) & ~(int64_t)255;
        tbase[sl] = cap_total; cap_total += cap[sl];
    }
    uint8_t *dq, *dr; int64_t *dqo, *dro, *dtoff; pmx_record_t *drec; char *dtext;
    if (scratch_reserve(qbytes, (void **)&dq, SCR_HQ) || scratch_reserve(rbytes, (void **)&dr, SCR_HR) ||
        scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dqo, SCR_HQO) || scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dro, SCR_HRO) ||
        scratch_reserve(sizeof(pmx_record_t) * n, (void **)&drec, SCR_HREC) ||
        scratch_reserve((size_t)cap_total, (void **)&dtext, SCR_HTEXT) ||
        scratch_reserve(sizeof(int64_t) * (n + K), (void **)&dtoff, SCR_HTOFF)) return -1;
    HIP_OR_RET(hipMemcpyAsync(dqo, qoff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    HIP_OR_RET(hipMemcpyAsync(dro, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = lo[sl], e = hi[sl];
        if (e <= a) continue;
        HIP_OR_RET(hipMemcpyAsync(dq + qoff[a], qbuf + qoff[a], (size_t)(qoff[e] - qoff[a]), hipMemcpyHostToDevice, s_copy));
        HIP_OR_RET(hipMemcpyAsync(dr + roff[a], rbuf + roff[a], (size_t)(roff[e] - roff[a]), hipMemcpyHostToDevice, s_copy));
        HIP_OR_RET(hipEventRecord(s_up[sl], s_copy));
        HIP_OR_RET(hipStreamWaitEvent(s_comp, s_up[sl], 0));
        const int rc = cigar_device_run(cfg, dm, e - a, dq, dqo + a, dr, dro + a, mq, mr, (long long)(qoff[a] + roff[a]),
                                        drec + a, dtext + tbase[sl], cap[sl], dtoff + a + sl, s_comp);
        if (rc) { (void)hipStreamSynchronize(s_comp); return rc; }
        HIP_OR_RET(hipEventRecord(s_done[sl], s_comp));
    }
    tm.done("queue H2D + kernels");
    std::vector<int64_t> toff;
    for (int sl = 0; sl < K; ++sl) {
        const int64_t a = lo[sl], e = hi[sl], m = e - a;
        if (m <= 0) continue;
        HIP_OR_RET(hipEventSynchronize(s_done[sl]));
        toff.resize((size_t)m + 1);
        HIP_OR_RET(hipMemcpy(toff.data(), dtoff + a + sl, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost));
        HIP_OR_RET(hipMemcpy(out + a, drec + a, sizeof(pmx_record_t) * m, hipMemcpyDeviceToHost));
        const int64_t total = toff[m];
        char *dst = text.grow((size_t)total);
        if (!dst) { (void)hipStreamSynchronize(s_comp); set_err("out of memory"); return -1; }
        if (total > cap[sl]) {
            // rare: the slice's text did not fit its share; every later slice has to finish first (the ops scratch is reused per slice),
            // so redo this slice alone with an exact-size text buffer
            HIP_OR_RET(hipStreamSynchronize(s_comp));
            DevBuf<char> big; DevBuf<int64_t> boff;
            if (big.try_alloc((size_t)total + 1) || boff.try_alloc((size_t)m + 1)) { set_err("out of device memory"); return -1; }
            const int rc = cigar_device_run(cfg, dm, m, dq, dqo + a, dr, dro + a, mq, mr, (long long)(qoff[a] + roff[a]),
                                            drec + a, big.p, total, boff.p, s_comp);
            if (rc) return rc < 0 ? rc : -1;
            HIP_OR_RET(hipStreamSynchronize(s_comp));
            HIP_OR_RET(hipMemcpy(dst, big.p, (size_t)total, hipMemcpyDeviceToHost));
        } else if (total) {
            HIP_OR_RET(hipMemcpy(dst, dtext + tbase[sl], (size_t)total, hipMemcpyDeviceToHost));
        }
        const int64_t base = (int64_t)text.len;
        for (int64_t k = 0; k < m; ++k) cigar_off[a + k + 1] = base + toff[k + 1];
        text.len += (size_t)total;
    }
    tm.done("kernels + D2H");
    return 0;
}

extern "C" int pmx_align_batch_cigar(const pmx_config_t *cfg, int64_t n,
                                     const uint8_t *qbuf, const int64_t *qoff,
                                     const uint8_t *rbuf, const int64_t *roff,
                                     pmx_record_t *out, char **cigar_buf, int64_t *cigar_off)
{
    if (check_cfg(cfg)) return -1;
    if (!cigar_buf || !cigar_off) { set_err("null cigar output"); return -1; }
    *cigar_buf = nullptr;
    if (n <= 0) return 0;
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {           // (the general trace table + pmx_walk_kernel: it reads no score)
        int32_t mq = 0, mnq = 0; bool bad = false;
        host_maxlens(n, qoff, &mq, &bad, &mnq);
        if (pssm_batch_check(cfg->matrix, mnq, mq)) return -1;
    }
    if (qoff[0] != 0 || roff[0] != 0) { set_err("offset arrays must start at 0"); return -1; }
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    TextBuf text;
    cigar_off[0] = 0;
    {
        const int rc = cigar_host_pipelined(cfg, dm, n, qbuf, qoff, rbuf, roff, out, text, cigar_off);
        if (rc < 0) { free(text.p); return rc; }
        if (rc == 0) return publish_text(text, cigar_buf);
    }
    // Chunks bound the per-launch trace scratch: budgeted at one byte per cell of the padded tables (the
    // general kernel's layout; the fast kernels write 4 bits per cell).  Large chunks matter: the walk is one
    // lane per pair and hides its dependent-load latency only with many waves in flight.  Up to 96 GB,
    // at most 45 % of the free HBM.
    const double chunk_bytes = chunk_budget(96e9, 0.45, pmx_env("PMX_CIGAR_CHUNK_BYTES"));
    // equal shares: as many chunks as the budget needs, each with about the same number of table bytes
    double total_bytes = 0;
    for (int64_t k = 0; k < n; ++k) total_bytes += 1.0 * (double)(qoff[k + 1] - qoff[k] + 64) * (double)(roff[k + 1] - roff[k] + 64);
    const double nchunks = total_bytes > chunk_bytes ? (double)(int64_t)(total_bytes / chunk_bytes + 1.0) : 1.0;
    const double share = total_bytes / nchunks + 1.0;
    int64_t c0 = 0;
    while (c0 < n) {
        int64_t c1 = c0; double bytes = 0;
        while (c1 < n && (c1 == c0 || bytes < share)) {
            bytes += 1.0 * (double)(qoff[c1 + 1] - qoff[c1] + 64) * (double)(roff[c1 + 1] - roff[c1] + 64);
            ++c1;
        }
        const int64_t m = c1 - c0;
        std::vector<int64_t> qo(m + 1), ro(m + 1);
        for (int64_t k = 0; k <= m; ++k) { qo[k] = qoff[c0 + k] - qoff[c0]; ro[k] = roff[c0 + k] - roff[c0]; }
        const int rc = cigar_chunk(cfg, dm, m, qbuf + qoff[c0], qo.data(), rbuf + roff[c0], ro.data(),
                                   out + c0, text, cigar_off + c0);
        if (rc) { free(text.p); return rc; }
        c0 = c1;
    }
    return publish_text(text, cigar_buf);
}

// ---- what the traced entries (banded, long pairs) share around their device routines -------------------------------------------
// cfg->want of a traced entry: CIGAR and / or statistics, nothing unknown.  `who` opens the message.
static int traced_want_check(const pmx_config_t *cfg, const char *who)
{
    if (!(cfg->want & (PMX_WANT_CIGAR | PMX_WANT_STATS))) { set_err("%s needs PMX_WANT_CIGAR and / or PMX_WANT_STATS in cfg->want", who); return -1; }
    if (cfg->want & ~(PMX_WANT_CIGAR | PMX_WANT_STATS | PMX_WANT_SORTED)) { set_err("unknown want bits 0x%x", cfg->want); return -1; }
    return 0;
}
// An output for everything cfg->want asks for.  A call that lacks both is told about the statistics buffer by the device entries
// and about the text by the host entries (text_first).
static int traced_outputs_check(const pmx_config_t *cfg, const void *stats, const void *text, const void *text_off, bool text_first)
{
    const bool no_stats = (cfg->want & PMX_WANT_STATS) && !stats, no_text = (cfg->want & PMX_WANT_CIGAR) && (!text || !text_off);
    if (no_text && (text_first || !no_stats)) { set_err("null cigar output"); return -1; }
    if (no_stats) { set_err("stats requested without a stats buffer"); return -1; }
    return 0;
}

// Host entry of a traced batch: host buffers in, host records / statistics / CIGAR text out (the text as pmx_align_batch_cigar's: a
// block freed with pmx_free).  run(staged batch, d_stats, d_text, capacity, d_text_off) is the device entry; it returns once the
// device is done with the batch.
template <typename Run>
static int traced_host_batch(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                             const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff, const int32_t *diag,
                             pmx_record_t *out, pmx_stats_t *stats_out, char **cigar_buf, int64_t *cigar_off, Run run)
{
    const bool want_cigar = (cfg->want & PMX_WANT_CIGAR) != 0, want_stats = (cfg->want & PMX_WANT_STATS) != 0;
    StagedBatch s;
    int rc = s.upload(profile, n, qbuf, qoff, rbuf, roff, diag);
    if (rc) return rc;
    const int64_t qbytes = profile ? (int64_t)n * profile->s1Len : qoff[n];
    // text capacity: half a byte per symbol + 16 per pair covers related pairs many times over; a batch that needs more runs again
    DevBuf<pmx_stats_t> dst; HostText text;
    if (want_stats && dst.try_alloc(n)) { set_err("out of device memory"); return -2; }
    if (want_cigar && text.alloc(n, (qbytes + roff[n]) / 2 + 16 * n + 256)) return -2;
    rc = text.run(n, cigar_off, nullptr, [&](char *d_text, int64_t capacity, int64_t *d_text_off) { return run(s, dst.p, d_text, capacity, d_text_off); });
    if (rc) return rc;
    if ((rc = s.records(out)) != 0) return rc;
    if (want_stats) HIP_OR_RET(hipMemcpy(stats_out, dst.p, sizeof(pmx_stats_t) * n, hipMemcpyDeviceToHost));
    return want_cigar ? text.to_block(cigar_off[n], cigar_buf) : 0;
}

// ---- banded batches with traceback (extension) ---------------------------------------------------------------------------
// The trace form of the 32-bit banded kernels (pmx_banded.hip) writes the band's decision bits to HBM scratch in the anti-diagonal
// layout of pmx_common.h, and pmx_walkb_kernel (pmx_walkb.hip) walks them: run-length ops into the per-pair slots of the device CIGAR
// entry, and / or the path's statistics.  Same band rule, records and oracle as banded_device.
static int banded_trace_check(const pmx_config_t *cfg, int32_t band)
{
    if (check_cfg(cfg)) return -1;
    if (band < 0 || band > 63) { set_err("banded traceback supports bands 0 .. 63 (got %d)", band); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) { set_err("PSSM matrices are not supported by banded batches"); return -1; }
    if (cfg->matrix->size > PMX_MAX_FAST_MSIZE) { set_err("banded traceback supports alphabets of up to %d letters (matrix size %d)", PMX_MAX_FAST_MSIZE, cfg->matrix->size); return -1; }
    return traced_want_check(cfg, "banded traceback");
}

// Validated by the caller.  d_qoff is NULL with one shared query of q_shared bytes; offsets start at 0.  Asynchronous on `st`.
static int banded_trace_device(const pmx_config_t *cfg, int64_t n, const uint8_t *d_qbuf, const int64_t *d_qoff, int q_shared,
                               const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_qlen, int32_t max_rlen,
                               int32_t band, const int32_t *d_diag, pmx_record_t *d_out, pmx_stats_t *d_stats,
                               char *d_text, int64_t capacity, int64_t *d_text_off, hipStream_t st,
                               int32_t *d_beg = nullptr /* two ints per pair: the first cell of each path (the search entries) */)
{
    const bool want_cigar = (cfg->want & PMX_WANT_CIGAR) != 0, want_stats = (cfg->want & PMX_WANT_STATS) != 0;
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    if (trace_ws_init()) return -1;
    const PmxBandTrGeometry g = pmx_bandtr_geometry_of(max_qlen, max_rlen, band);
    // chunks as in cigar_device_run: at most ~12 GB of trace each (two buffers), at most 15 % of the free HBM, two once it pays
    const double chunk_bytes = chunk_budget(12e9, 0.15, pmx_env("PMX_CIGAR_CHUNK_BYTES"));
    // The walk (one lane per pair) costs about what the sweep does and only the last chunk's walk is exposed: eight chunks once the
    // batch is worth it (measured on 1.25 M pairs of 250 x 250, band 15: two chunks 24.3 ms, nine 20.5 ms)
    const int64_t chunk = chunk_pairs(n, (double)n * (double)g.stride, chunk_bytes, n >= 8 * 16384 ? 8 : n >= 16384 ? 2 : 1);
    const bool two = chunk < n;
    const size_t cbytes = ((size_t)chunk * (size_t)g.stride + 255) & ~(size_t)255;
    uint8_t *tbuf = nullptr; SlotText t; int64_t *slot_qoff = nullptr;
    if (scratch_reserve(cbytes * (two ? 2 : 1), (void **)&tbuf, SCR_TRACE) ||
        (want_cigar && t.reserve_ops((size_t)n * ((size_t)max_qlen + max_rlen + 1))) ||
        scratch_carve(SCR_CIG, [&](Carver &c) { t.carve(c, n, want_cigar); slot_qoff = c.take<int64_t>((size_t)n + 1); })) return -1;
    if (want_cigar && q_shared) {                 // the slot render finds a slot from query offsets: k * qlen for the shared query
        const int rc = pmx_launch_shared_offsets(slot_qoff, n, q_shared, st);
        if (rc) { set_err("offset kernel launch failed (%d)", rc); return rc; }
    }
    const int64_t *sq = q_shared ? slot_qoff : d_qoff;
    const char *kname = "pmx_banded_kernel/trace";
    int rc = overlap_chunks(n, chunk, two, st, [&](const ChunkTurn &k) -> int {
        const int64_t c0 = k.c0, m = k.n;
        const PmxBandTrace tr = {tbuf + (size_t)k.buf * cbytes, g.stride};
        const int64_t *qo = d_qoff ? d_qoff + c0 : nullptr;
        const int32_t *dg = d_diag ? d_diag + c0 : nullptr;
        int rc = pmx_launch_banded_trace(cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, dm.d, m, d_qbuf, qo, q_shared, d_rbuf, d_roff + c0,
                                         max_qlen, max_rlen, band, dg, d_out + c0, tr, k.sweep, &kname);
        if (rc) { set_err("banded trace launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        if ((rc = chunk_sweep_launched(k)) != 0) return rc;
        if (want_stats)
            rc = pmx_launch_walkb(cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, dm.d, m, d_qbuf, qo, q_shared, d_rbuf, d_roff + c0, band, dg,
                                  d_out + c0, tr, nullptr, 0, nullptr, nullptr, nullptr, d_stats + c0, k.walk, d_beg ? d_beg + 2 * c0 : nullptr);
        if (!rc && want_cigar)
            rc = pmx_launch_walkb(cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, dm.d, m, d_qbuf, qo, q_shared, d_rbuf, d_roff + c0, band, dg,
                                  d_out + c0, tr, sq + c0, -c0, t.ops, t.nops + c0, t.textlen + c0, nullptr, k.walk,
                                  d_beg && !want_stats ? d_beg + 2 * c0 : nullptr);
        if (rc) { set_err("banded walk launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        return chunk_walk_launched(k);
    });
    if (!rc && want_cigar) rc = t.render(sq, d_roff, 0, n, d_text, capacity, d_text_off, st);
    if (rc) return rc;
    g_last_kernel = strcmp(kname, "pmx_banded_staged_kernel/trace") == 0 ? "pmx_banded_staged_kernel/trace + pmx_walkb_kernel"
                                                                          : "pmx_banded_kernel/trace + pmx_walkb_kernel";
    return 0;
}

extern "C" int pmx_align_batch_banded_cigar_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                                   const uint8_t *d_qbuf, const int64_t *d_qoff, const uint8_t *d_rbuf, const int64_t *d_roff,
                                                   int32_t max_qlen, int32_t max_rlen, int32_t band, const int32_t *d_diag,
                                                   pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                                                   char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, void *stream)
{
    if (banded_trace_check(cfg, band)) return -1;
    if (n <= 0) return 0;
    if (profile && profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    if (!d_rbuf || !d_roff || !d_out || (!profile && (!d_qbuf || !d_qoff))) { set_err("null buffer"); return -1; }
    if (traced_outputs_check(cfg, d_stats_out, d_cigar_text, d_cigar_off, false)) return -1;
    if ((!profile && max_qlen <= 0) || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    const uint8_t *dq = d_qbuf;
    if (profile && profile_device_query(profile, &dq)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return banded_trace_device(cfg, n, dq, profile ? nullptr : d_qoff, profile ? profile->s1Len : 0, d_rbuf, d_roff,
                               profile ? profile->s1Len : max_qlen, max_rlen, band, d_diag, d_out, d_stats_out,
                               d_cigar_text, cigar_capacity, d_cigar_off, (hipStream_t)stream);
}

// Host buffers in, host records / statistics / CIGAR text out (the text as pmx_align_batch_cigar's: a block freed with pmx_free).
extern "C" int pmx_align_batch_banded_cigar(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                            const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                            int32_t band, const int32_t *diag,
                                            pmx_record_t *out, pmx_stats_t *stats_out, char **cigar_buf, int64_t *cigar_off)
{
    if (banded_trace_check(cfg, band) || traced_outputs_check(cfg, stats_out, cigar_buf, cigar_off, true)) return -1;
    if (cfg->want & PMX_WANT_CIGAR) *cigar_buf = nullptr;
    if (n <= 0) return 0;
    if (!rbuf || !roff || !out || (!profile && (!qbuf || !qoff))) { set_err("null buffer"); return -1; }
    if (profile && profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    return traced_host_batch(cfg, profile, n, qbuf, qoff, rbuf, roff, diag, out, stats_out, cigar_buf, cigar_off,
        [&](const StagedBatch &s, pmx_stats_t *d_stats, char *d_text, int64_t capacity, int64_t *d_text_off) -> int {
            const int rc = pmx_align_batch_banded_cigar_device(cfg, profile, n, s.dq.p, s.dqo.p, s.dr.p, s.dro.p, s.mq, s.mr, band, s.dd.p,
                                                               s.drec.p, d_stats, d_text, capacity, d_text_off, nullptr);
            if (rc) return rc;
            HIP_OR_RET(hipDeviceSynchronize());
            return 0;
        });
}

// ==================================================================== profile database search ===
// pmx_search_profile[_device]: the score-only first pass of pmx_align_profile_batch_device, the selection and the gather of
// pmx_select.hip, the banded trace road above in its profile arm over the gathered hits (diag = end_ref - end_query of the first
// pass), and the begins pmx_walkb_kernel leaves.  One stream synchronisation, between the passes: the host has to know the number of
// hits and of their reference bytes to size the second pass.
extern "C" int pmx_select_hits_device(const pmx_record_t *d_rec, int64_t n, int32_t min_score, int64_t max_hits, int order,
                                      int64_t *d_hit_index, int64_t capacity, int64_t *d_counts, void *stream)
{
    if (n < 0 || max_hits < 0 || capacity < 0) { set_err("negative n, max_hits or capacity"); return -1; }
    if (order != PMX_HITS_BY_INDEX && order != PMX_HITS_BY_SCORE) { set_err("bad hit order %d", order); return -1; }
    if (!d_counts || (n > 0 && !d_rec) || (n > 0 && capacity > 0 && !d_hit_index)) { set_err("null buffer"); return -1; }
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    void *scr = nullptr;
    if (scratch_reserve(pmx_select_scratch_bytes(n, max_hits, order), &scr, SCR_SEL)) return -1;
    const int rc = pmx_launch_select(d_rec, n, min_score, max_hits, order, d_hit_index, capacity, d_counts, scr, (hipStream_t)stream);
    if (rc) { set_err("hit selection failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
    return 0;
}

extern "C" int pmx_gather_refs_device(const uint8_t *d_rbuf, const int64_t *d_roff, int64_t n, const int64_t *d_index, int64_t h,
                                      uint8_t *d_out, int64_t out_capacity, int64_t *d_out_off, void *stream)
{
    if (n < 0 || h < 0 || out_capacity < 0) { set_err("negative n, h or out_capacity"); return -1; }
    if (!d_out_off || (h > 0 && (!d_rbuf || !d_roff || !d_index || !d_out))) { set_err("null buffer"); return -1; }
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    int32_t *hlen = nullptr; void *scan = nullptr; const size_t scan_bytes = pmx_text_scan_scratch_bytes(h);
    if (scratch_carve(SCR_SRCH, [&](Carver &c) { hlen = c.take<int32_t>((size_t)h + 2); scan = c.take<unsigned char>(scan_bytes); })) return -1;
    int rc = pmx_launch_hit_lengths(d_index, nullptr, h, nullptr, d_roff, nullptr, hlen, st);
    if (!rc) rc = pmx_launch_text_offsets(hlen, h, d_out_off, scan, scan_bytes, st);
    if (!rc) rc = pmx_launch_gather_refs(d_rbuf, d_roff, n, d_index, h, d_out, d_out_off, out_capacity, st);
    if (rc) { set_err("reference gather failed (%d)", rc); return rc; }
    return 0;
}

// Everything a search refuses, before any GPU work.
static int search_check(const pmx_config_t *cfg, const parasail_profile_t *profile, const pmx_search_opts_t *opts, int64_t n, int64_t capacity)
{
    if (check_cfg(cfg)) return -1;
    if (!profile) { set_err("null profile"); return -1; }
    if (!opts) { set_err("null search options"); return -1; }
    if (n < 0) { set_err("negative n"); return -1; }
    if (opts->order != PMX_HITS_BY_INDEX && opts->order != PMX_HITS_BY_SCORE) { set_err("bad hit order %d", opts->order); return -1; }
    if (opts->max_hits < 0) { set_err("negative max_hits"); return -1; }
    if (capacity < 0) { set_err("negative hit capacity"); return -1; }
    if (opts->band > 63) { set_err("the second pass of a search supports bands 0 .. 63 (got %d); band < 0: none", opts->band); return -1; }
    if (opts->band >= 0 && banded_trace_check(cfg, opts->band)) return -1;
    if (cfg->want & ~(PMX_WANT_CIGAR | PMX_WANT_STATS | PMX_WANT_SORTED)) { set_err("unknown want bits 0x%x", cfg->want); return -1; }
    if (profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    return pssm_batch_check(cfg->matrix, profile->s1Len, profile->s1Len);
}

// The hit list of a search on the device, between selection and second pass.  cap: the most hits that can be listed.
struct SearchHits {
    int64_t cap = 0, *idx = nullptr, *roff = nullptr, *counts = nullptr; int32_t *diag = nullptr, *hlen = nullptr, *beg = nullptr;
    void *scan = nullptr; size_t scan_bytes = 0;
    int64_t selected = 0, passing = 0, h = 0, bytes = 0;      // read back: counts, hits listed, their reference bytes
};
static thread_local int64_t *g_search_pin = nullptr;          // three int64 of page-locked memory for that read-back

// Selection over the first pass's records, hit diagonals / lengths / offsets, and the one synchronisation.  d_counts: the caller's
// counts, or NULL.
static int search_select(int64_t n, const pmx_record_t *d_first, const int64_t *d_roff, const pmx_search_opts_t *opts, int64_t capacity,
                         int64_t *d_counts, hipStream_t st, SearchHits *sh)
{
    sh->cap = std::min<int64_t>(std::min<int64_t>(n, capacity), opts->max_hits > 0 ? opts->max_hits : n);
    const int64_t cap = sh->cap;
    sh->scan_bytes = pmx_text_scan_scratch_bytes(cap);
    void *sel = nullptr;
    if (scratch_reserve(pmx_select_scratch_bytes(n, opts->max_hits, opts->order), &sel, SCR_SEL) ||
        scratch_carve(SCR_SRCH, [&](Carver &c) {
            sh->idx = c.take<int64_t>((size_t)cap); sh->roff = c.take<int64_t>((size_t)cap + 1); sh->counts = c.take<int64_t>(2);
            sh->diag = c.take<int32_t>((size_t)cap); sh->hlen = c.take<int32_t>((size_t)cap + 2); sh->beg = c.take<int32_t>(2 * (size_t)cap);
            sh->scan = c.take<unsigned char>(sh->scan_bytes);
        })) return -1;
    if (!g_search_pin) HIP_OR_RET(hipHostMalloc((void **)&g_search_pin, 3 * sizeof(int64_t), hipHostMallocDefault));
    int64_t *counts = d_counts ? d_counts : sh->counts;
    int rc = pmx_launch_select(d_first, n, opts->min_score, opts->max_hits, opts->order, sh->idx, cap, counts, sel, st);
    if (!rc) rc = pmx_launch_hit_lengths(sh->idx, counts, cap, d_first, d_roff, sh->diag, sh->hlen, st);
    if (!rc) rc = pmx_launch_text_offsets(sh->hlen, cap, sh->roff, sh->scan, sh->scan_bytes, st);
    if (rc) { set_err("hit selection failed (%d)", rc); return rc; }
    HIP_OR_RET(hipMemcpyAsync(g_search_pin, counts, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipMemcpyAsync(g_search_pin + 2, sh->roff + cap, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    sh->selected = g_search_pin[0]; sh->passing = g_search_pin[1]; sh->bytes = g_search_pin[2];
    sh->h = std::min<int64_t>(sh->selected, cap);
    return 0;
}

// The hit records and, with band >= 0, the second pass over the gathered references.  Asynchronous on `st`; may be run again (a
// larger text buffer).
static int search_second(const pmx_config_t *cfg, const parasail_profile_t *profile, const uint8_t *dq, int64_t n,
                         const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen, const pmx_search_opts_t *opts,
                         const pmx_record_t *d_first, const SearchHits &sh, pmx_hit_t *d_hits, pmx_record_t *d_recs, pmx_stats_t *d_stats,
                         char *d_text, int64_t text_capacity, int64_t *d_text_off, hipStream_t st)
{
    const int64_t h = sh.h;
    int rc = pmx_launch_hit_records(sh.idx, d_first, sh.diag, h, d_hits, st);
    if (rc) { set_err("hit record launch failed (%d)", rc); return rc; }
    if (opts->band < 0 || h == 0) {
        if (d_text_off) HIP_OR_RET(hipMemsetAsync(d_text_off, 0, sizeof(int64_t) * (size_t)(h + 1), st));
        return 0;
    }
    uint8_t *gref = nullptr;
    if (scratch_reserve((size_t)sh.bytes + 16, (void **)&gref, SCR_GREF)) return -1;      // (the padding of the host entries' staged references)
    rc = pmx_launch_gather_refs(d_rbuf, d_roff, n, sh.idx, h, gref, sh.roff, sh.bytes, st);
    if (rc) { set_err("reference gather failed (%d)", rc); return rc; }
    const char *first_kernel = g_last_kernel;
    rc = banded_trace_device(cfg, h, dq, nullptr, profile->s1Len, gref, sh.roff, profile->s1Len, max_rlen, opts->band, sh.diag,
                             d_recs, d_stats, d_text, text_capacity, d_text_off, st, sh.beg);
    if (rc) return rc;
    static thread_local char name[256];
    if (first_kernel != name) {
        char both[256];
        snprintf(both, sizeof both, "%s + pmx_select + pmx_gather_refs_kernel + %s", first_kernel, g_last_kernel);
        memcpy(name, both, sizeof name);
    }
    g_last_kernel = name;
    rc = pmx_launch_hit_begins(sh.beg, h, d_hits, st);
    if (rc) { set_err("hit begin launch failed (%d)", rc); return rc; }
    return 0;
}

extern "C" int pmx_search_profile_device(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                         const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_rlen, const pmx_search_opts_t *opts,
                                         pmx_record_t *d_first, pmx_hit_t *d_hits, pmx_record_t *d_recs, pmx_stats_t *d_stats, int64_t capacity,
                                         char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, int64_t *d_counts, void *stream)
{
    if (search_check(cfg, profile, opts, n, capacity)) return -1;
    if (!d_counts || (capacity > 0 && !d_hits)) { set_err("null buffer"); return -1; }
    const bool second = opts->band >= 0;
    if (second && capacity > 0 && (!d_recs || traced_outputs_check(cfg, d_stats, d_cigar_text, d_cigar_off, false))) {
        if (!d_recs) set_err("null buffer");
        return -1;
    }
    if (second && cigar_capacity < 0) { set_err("negative cigar_capacity"); return -1; }
    if (n > 0 && (!d_rbuf || !d_roff)) { set_err("null buffer"); return -1; }
    if (n > 0 && max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    if (n == 0) {
        HIP_OR_RET(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), st));
        if (d_cigar_off) HIP_OR_RET(hipMemsetAsync(d_cigar_off, 0, sizeof(int64_t), st));
        return 0;
    }
    const uint8_t *dq = nullptr;
    if (profile_device_query(profile, &dq)) return -1;
    if (!d_first && scratch_reserve(sizeof(pmx_record_t) * (size_t)n, (void **)&d_first, SCR_HREC)) return -1;
    pmx_config_t cfg1 = *cfg;
    cfg1.want &= PMX_WANT_SORTED;
    int rc = run_batch_device(&cfg1, n, dq, nullptr, profile->s1Len, d_rbuf, d_roff, profile->s1Len, max_rlen, d_first, nullptr, stream,
                              profile_has_wildcard(profile));
    if (rc) return rc;
    SearchHits sh;
    if ((rc = search_select(n, d_first, d_roff, opts, capacity, d_counts, st, &sh)) != 0) return rc;
    return search_second(cfg, profile, dq, n, d_rbuf, d_roff, max_rlen, opts, d_first, sh, d_hits, d_recs, d_stats,
                         d_cigar_text, cigar_capacity, d_cigar_off, st);
}

extern "C" void pmx_search_result_free(pmx_search_result_t *result) { free(result); }

extern "C" int pmx_search_profile(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                  const uint8_t *rbuf, const int64_t *roff, const pmx_search_opts_t *opts, pmx_search_result_t **result)
{
    if (!result) { set_err("null result pointer"); return -1; }
    *result = nullptr;
    if (search_check(cfg, profile, opts, n, 0)) return -1;
    if (n > 0 && (!rbuf || !roff)) { set_err("null buffer"); return -1; }
    const bool second = opts->band >= 0;
    const bool want_cigar = second && (cfg->want & PMX_WANT_CIGAR), want_stats = second && (cfg->want & PMX_WANT_STATS);
    // the result: one block -- header, hits, records, statistics, offsets, text
    auto publish = [&](int64_t h, int64_t passing, int64_t text_bytes, pmx_search_result_t **out) -> int {
        auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
        const size_t o_hits = up(sizeof(pmx_search_result_t)), o_recs = o_hits + up(sizeof(pmx_hit_t) * (size_t)h);
        const size_t o_stats = o_recs + (second ? up(sizeof(pmx_record_t) * (size_t)h) : 0);
        const size_t o_off = o_stats + (want_stats ? up(sizeof(pmx_stats_t) * (size_t)h) : 0);
        const size_t o_text = o_off + up(sizeof(int64_t) * (size_t)(h + 1)), total = o_text + (want_cigar ? (size_t)text_bytes + 1 : 0);
        char *blk = (char *)calloc(1, total);
        if (!blk) { set_err("out of memory"); return -1; }
        pmx_search_result_t *r = (pmx_search_result_t *)blk;
        r->n_hits = h; r->n_passing = passing;
        r->hits = (pmx_hit_t *)(blk + o_hits);
        r->recs = second ? (pmx_record_t *)(blk + o_recs) : nullptr;
        r->stats = want_stats ? (pmx_stats_t *)(blk + o_stats) : nullptr;
        r->cigar_off = (int64_t *)(blk + o_off);
        r->cigar = want_cigar ? blk + o_text : nullptr;
        *out = r;
        return 0;
    };
    if (n == 0) return publish(0, 0, 0, result);
    int32_t mr = 0, mnr = 0; bool bad = false;
    host_maxlens(n, roff, &mr, &bad, &mnr);
    if (bad || roff[0] != 0) { set_err("bad reference offsets"); return -1; }
    pmx_config_t cfg1 = with_sort_hint(cfg, mnr, mr, n);
    cfg1.want &= PMX_WANT_SORTED;
    const uint8_t *dq = nullptr;
    if (profile_device_query(profile, &dq)) return -1;
    // the references go up once, in slices behind which the first pass runs (as in pmx_align_profile_batch), and stay for the gather
    const size_t rbytes = (size_t)roff[n];
    uint8_t *dr = nullptr; int64_t *dro = nullptr; pmx_record_t *dfirst = nullptr;
    if (scratch_reserve(rbytes + 16, (void **)&dr, SCR_HR) || scratch_reserve(sizeof(int64_t) * (n + 1), (void **)&dro, SCR_HRO) ||
        scratch_reserve(sizeof(pmx_record_t) * n, (void **)&dfirst, SCR_HREC)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t s_copy = hs.copy, s_comp = hs.comp;
    StreamGuard guard(s_comp);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const int K = rbytes >= ((size_t)64 << 20) ? (int)std::max<int64_t>(1, std::min<int64_t>(8, n / 32768)) : 1;
    HIP_OR_RET(hipMemcpyAsync(dro, roff, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s_copy));
    const int wild = profile_has_wildcard(profile);
    int64_t a = 0;
    for (int sl = 0; sl < K; ++sl) {
        int64_t e = n;
        if (sl + 1 < K) {
            e = std::lower_bound(roff, roff + n + 1, (int64_t)(rbytes / K) * (sl + 1)) - roff;
            e = std::min<int64_t>(std::max<int64_t>(e, a), n);
        }
        if (e <= a) continue;
        HIP_OR_RET(hipMemcpyAsync(dr + roff[a], rbuf + roff[a], (size_t)(roff[e] - roff[a]), hipMemcpyHostToDevice, s_copy));
        HIP_OR_RET(hipEventRecord(hs.up[sl], s_copy));
        HIP_OR_RET(hipStreamWaitEvent(s_comp, hs.up[sl], 0));
        const int rc = run_batch_device(&cfg1, e - a, dq, nullptr, profile->s1Len, dr, dro + a, profile->s1Len, mr, dfirst + a, nullptr, s_comp, wild);
        if (rc) { (void)hipStreamSynchronize(s_comp); (void)hipStreamSynchronize(s_copy); return rc; }
        a = e;
    }
    SearchHits sh;
    int rc = search_select(n, dfirst, dro, opts, n, nullptr, s_comp, &sh);
    if (rc) { (void)hipStreamSynchronize(s_comp); return rc; }
    const int64_t h = sh.h;
    // text capacity as in traced_host_batch: half a byte per symbol + 16 per hit; a search that needs more runs its second pass again
    DevBuf<pmx_hit_t> dhits; DevBuf<pmx_record_t> drecs; DevBuf<pmx_stats_t> dst; HostText text;
    if (dhits.try_alloc(h) || (second && drecs.try_alloc(h)) || (want_stats && dst.try_alloc(h))) { set_err("out of device memory"); return -2; }
    if (want_cigar && text.alloc(h, ((int64_t)h * profile->s1Len + sh.bytes) / 2 + 16 * h + 256)) return -2;
    std::vector<int64_t> toff((size_t)h + 1, 0);
    rc = text.run(h, toff.data(), nullptr, [&](char *d_text, int64_t capacity, int64_t *d_text_off) -> int {
        const int rc2 = search_second(cfg, profile, dq, n, dr, dro, mr, opts, dfirst, sh, dhits.p, drecs.p, dst.p, d_text, capacity, d_text_off, s_comp);
        if (rc2) { (void)hipStreamSynchronize(s_comp); return rc2; }
        HIP_OR_RET(hipStreamSynchronize(s_comp));
        return 0;
    });
    if (rc) return rc;
    pmx_search_result_t *r = nullptr;
    if (publish(h, sh.passing, toff[h], &r)) return -1;
    hipError_t e = hipSuccess;
    if (h) {
        e = hipMemcpy(r->hits, dhits.p, sizeof(pmx_hit_t) * (size_t)h, hipMemcpyDeviceToHost);
        if (e == hipSuccess && second) e = hipMemcpy(r->recs, drecs.p, sizeof(pmx_record_t) * (size_t)h, hipMemcpyDeviceToHost);
        if (e == hipSuccess && want_stats) e = hipMemcpy(r->stats, dst.p, sizeof(pmx_stats_t) * (size_t)h, hipMemcpyDeviceToHost);
        if (e == hipSuccess && want_cigar) e = text.copy_to(r->cigar, toff[h]);
    }
    if (e != hipSuccess) { free(r); set_err("%s", hipGetErrorString(e)); return -(int)e; }
    memcpy(r->cigar_off, toff.data(), sizeof(int64_t) * (size_t)(h + 1));
    *result = r;
    return 0;
}

// ==================================================================== long pairs: traceback in linear memory ===
// pmx_align_batch_cigar_long: the checkpoint form of the long-pair sweep (pmx_long.hip, CK) keeps the row granules it hands from band
// to band anyway plus the (H, E) of every tile_cols-th column; pmx_walkt_kernel (pmx_walkt.hip) re-derives, from the end cell
// backwards, only the tiles the path enters.  Nothing is proportional to qlen x rlen: per pair 8 bytes per column and band, 8 bytes per
// row and column tile, 4 bytes per op slot.  Chunks of pairs share one scratch; sweep and walk of a chunk run back to back on the
// caller's stream, so a chunk's checkpoints live until its walk is done and the next chunk's sweep starts behind it.
static const int LONGCIG_DEFAULT_TILE = 128;
// The checkpoint road's sweep for n pairs: 0 fine, -1 refused with a message.  A single pair always gets the scratch it needs.
static int longcig_plan(int64_t n, int32_t max_qlen, int32_t max_rlen, int msize, const pmx_long_cigar_opts_t *opts, const LongKnobs &knobs, PmxLongPlan *pl)
{
    if (n <= 0 || max_qlen <= 0 || max_rlen <= 0) { set_err("n, max_qlen and max_rlen must be positive"); return -1; }
    int tile = opts ? opts->tile_cols : 0, rows = opts ? opts->band_rows : 0;
    if (tile == 0) tile = LONGCIG_DEFAULT_TILE;
    if (tile != 64 && tile != 128 && tile != 256) { set_err("tile_cols %d is not offered (64, 128, 256; 0 = default)", tile); return -1; }
    if (rows != 0 && rows != 128 && rows != 256 && rows != 1024) { set_err("band_rows %d is not offered (128, 256, 1024; 0 = the dispatcher's choice)", rows); return -1; }
    // two columns per step for a chunk of a few pairs (latency), one for a chunk that fills the chip (long_batch, measured)
    int R = rows ? rows / 64 : 4, cols_many = 1, cols_few = 2;
    long_apply_switches(knobs, false, &R, &cols_many);
    long_apply_switches(knobs, false, &R, &cols_few);
    PmxLongWant w = {};
    w.n = n; w.max_qlen = max_qlen; w.max_rlen = max_rlen; w.msize = msize; w.R = R; w.cols = cols_many; w.cols_few = cols_few;
    w.chunk_cols = knobs.chunk_cols; w.tile_cols = tile; w.budget = knobs.budget; w.refuse_above_budget = false; w.r16_above_4g = rows == 0;
    w.clamp_blocks = true;
    const int rc = pmx_long_plan(w, pl);
    if (rc) { set_err("the long-pair sweep does not take this configuration (alphabet above 64 letters, a profile beyond the LDS)"); return -1; }
    return 0;
}

extern "C" long long pmx_long_cigar_scratch_bytes(int64_t n, int32_t max_qlen, int32_t max_rlen, const pmx_long_cigar_opts_t *opts)
{
    PmxLongPlan pl;
    if (longcig_plan(n, max_qlen, max_rlen, 0, opts, long_env_knobs(), &pl)) return -1;
    return (long long)pl.total;
}

/* Test hook (include/parasail_amd.h): both roads' planning with the knobs as arguments; no device needed. */
extern "C" int pmx_long_plan_probe(int road, int mode, long long n, int max_qlen, int max_rlen, double budget, int budget_forced,
                                   int two_columns, int one_column, int rows_per_lane, int chunk_cols, int tile_cols, int band_rows, long long *out)
{
    LongKnobs knobs;
    knobs.two_columns = two_columns != 0; knobs.one_column = one_column != 0; knobs.rows_per_lane = rows_per_lane; knobs.chunk_cols = chunk_cols;
    knobs.budget = (size_t)budget; knobs.budget_forced = budget_forced != 0;
    const pmx_long_cigar_opts_t opts = {tile_cols, band_rows};
    PmxLongPlan pl = {};
    const int rc = road == 0 ? long_score_plan(mode, n, max_qlen, max_rlen, 4, knobs, &pl) : (longcig_plan(n, max_qlen, max_rlen, 4, &opts, knobs, &pl) ? 1 : 0);
    if (rc) pl = PmxLongPlan();
    const long long v[9] = {pl.R, pl.cols, pl.steps, pl.nbmax, pl.bstride, pl.pairs, (long long)pl.off_ck, (long long)pl.ck_bytes, pl.ckslots};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return rc;
}

static int long_cigar_check(const pmx_config_t *cfg, const pmx_long_cigar_opts_t *opts)
{
    if (check_cfg(cfg)) return -1;
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) { set_err("PSSM matrices are not supported by the tiled long-pair traceback"); return -1; }
    if (traced_want_check(cfg, "pmx_align_batch_cigar_long")) return -1;
    if (cfg->matrix->size > 64) { set_err("the long-pair kernels take alphabets of up to 64 letters (matrix size %d)", cfg->matrix->size); return -1; }
    PmxLongPlan pl;
    return longcig_plan(1, 1, 1, cfg->matrix->size, opts, LongKnobs(), &pl);          // (the options alone)
}

// Validated by the caller; offsets start at 0.  Asynchronous on `st`; *d_abort = the launch's abort word (device).
static int long_cigar_device(const pmx_config_t *cfg, int64_t n, const uint8_t *d_qbuf, const int64_t *d_qoff,
                             const uint8_t *d_rbuf, const int64_t *d_roff, int32_t max_qlen, int32_t max_rlen,
                             pmx_record_t *d_out, pmx_stats_t *d_stats, char *d_text, int64_t capacity, int64_t *d_text_off,
                             const pmx_long_cigar_opts_t *opts, hipStream_t st, const int **d_abort,
                             int64_t op_slots = 0 /* sum of qlen + rlen + 1 over the batch where the caller knows it; 0: n x the maxima */)
{
    const bool want_cigar = (cfg->want & PMX_WANT_CIGAR) != 0, want_stats = (cfg->want & PMX_WANT_STATS) != 0;
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    const LongKnobs knobs = long_knobs();
    PmxLongPlan pl;
    if (longcig_plan(n, max_qlen, max_rlen, dm.d.msize, opts, knobs, &pl)) return -1;
    unsigned char *scr = nullptr; SlotText t;
    if (scratch_reserve(pl.total, (void **)&scr, SCR_LONG) ||
        (want_cigar && t.reserve_ops(op_slots > 0 ? (size_t)op_slots : (size_t)n * ((size_t)max_qlen + max_rlen + 1))) ||
        scratch_carve(SCR_CIG, [&](Carver &c) { t.carve(c, n, want_cigar); })) return -1;
    HIP_OR_RET(hipMemsetAsync(scr + pl.off_abort, 0, pl.abort_bytes, st));
    for (int64_t c0 = 0; c0 < n; c0 += pl.pairs) {
        PmxBatch b; memset(&b, 0, sizeof b);
        b.qbuf = d_qbuf; b.qoff = d_qoff + c0; b.rbuf = d_rbuf; b.roff = d_roff + c0;
        b.n = (n - c0 < pl.pairs) ? n - c0 : pl.pairs; b.max_qlen = max_qlen; b.max_rlen = max_rlen;
        int rc = pmx_launch_long(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, pl, scr, d_out + c0, 2147483647, 0, knobs.spin_limit, st);
        if (rc < 0) { set_err("checkpoint sweep launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
        if (rc) { set_err("the long-pair sweep does not take this configuration (alphabet above 64 letters, scores or gap penalties beyond its 16-bit profile, lengths x penalties beyond 2^29)"); return -1; }
        rc = pmx_launch_walkt(b, dm.d, cfg->mode, cfg->sg_flags, cfg->open, cfg->extend, pl, scr, d_out + c0,
                              d_qoff + c0, -c0, t.ops, want_cigar ? t.nops + c0 : nullptr, want_cigar ? t.textlen + c0 : nullptr,
                              want_stats ? d_stats + c0 : nullptr, st);
        if (rc) { set_err("tile walk launch failed (%d)", rc); return rc < 0 ? rc : -1; }
    }
    if (want_cigar) {
        const int rc = t.render(d_qoff, d_roff, 0, n, d_text, capacity, d_text_off, st);
        if (rc) return rc;
    }
    if (d_abort) *d_abort = reinterpret_cast<const int *>(scr + pl.off_abort);
    g_last_kernel = pl.name;
    return 0;
}

extern "C" int pmx_align_batch_cigar_long_device(const pmx_config_t *cfg, int64_t n,
                                                 const uint8_t *d_qbuf, const int64_t *d_qoff, const uint8_t *d_rbuf, const int64_t *d_roff,
                                                 int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                                                 char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, void *stream,
                                                 const pmx_long_cigar_opts_t *opts)
{
    if (long_cigar_check(cfg, opts)) return -1;
    if (n <= 0) return 0;
    if (!d_qbuf || !d_qoff || !d_rbuf || !d_roff || !d_out) { set_err("null buffer"); return -1; }
    if (traced_outputs_check(cfg, d_stats_out, d_cigar_text, d_cigar_off, false)) return -1;
    if (max_qlen <= 0 || max_rlen <= 0) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return long_cigar_device(cfg, n, d_qbuf, d_qoff, d_rbuf, d_roff, max_qlen, max_rlen, d_out, d_stats_out,
                             d_cigar_text, cigar_capacity, d_cigar_off, opts, (hipStream_t)stream, nullptr);
}

extern "C" int pmx_align_batch_cigar_long(const pmx_config_t *cfg, int64_t n,
                                          const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                          pmx_record_t *out, pmx_stats_t *stats_out, char **cigar_buf, int64_t *cigar_off,
                                          const pmx_long_cigar_opts_t *opts)
{
    if (long_cigar_check(cfg, opts) || traced_outputs_check(cfg, stats_out, cigar_buf, cigar_off, true)) return -1;
    if (cfg->want & PMX_WANT_CIGAR) *cigar_buf = nullptr;
    if (n <= 0) return 0;
    if (!qbuf || !qoff || !rbuf || !roff || !out) { set_err("null buffer"); return -1; }
    return traced_host_batch(cfg, nullptr, n, qbuf, qoff, rbuf, roff, nullptr, out, stats_out, cigar_buf, cigar_off,
        [&](const StagedBatch &s, pmx_stats_t *d_stats, char *d_text, int64_t capacity, int64_t *d_text_off) -> int {
            const int *d_abort = nullptr;
            const int rc = long_cigar_device(cfg, n, s.dq.p, s.dqo.p, s.dr.p, s.dro.p, s.mq, s.mr, s.drec.p, d_stats, d_text, capacity, d_text_off,
                                             opts, nullptr, &d_abort, qoff[n] + roff[n] + n);
            if (rc) return rc;
            HIP_OR_RET(hipDeviceSynchronize());
            int gave_up = 0;
            HIP_OR_RET(hipMemcpy(&gave_up, d_abort, sizeof(int), hipMemcpyDeviceToHost));
            if (gave_up) {
                set_err("checkpoint sweep: a band's bounded wait for the band above ran out (dispatch order assumption broken, or PMX_LONG_SPIN_LIMIT); "
                        "no alignment is returned");
                return -3;
            }
            return 0;
        });
}

// ============================================================================= multi-GPU ===
// Pairs are independent (the reference's only parallel story is user threads sharing a read-only profile,
// tests/test_parasail.rs:689-723), so a batch shards across the GPUs of a node with no data-path collective: a contiguous block
// of pairs per device, cut so that every device gets about the same number of cells (sum of qlen * rlen), one host thread and one
// set of streams per device, results written straight into the caller's arrays in input order -- with one process driving all
// GPUs the per-device D2H copy IS the gather (one process per GPU + an RCCL gather: parasail-rs_amd/sharding.py, bench.py).
extern "C" int pmx_shard_bounds_by_cells(int64_t n, const int64_t *qoff /* NULL: one shared query */, const int64_t *roff,
                                         int parts, int64_t *bounds /* parts + 1 */)
{
    if (n < 0 || parts <= 0 || !roff || !bounds) return -1;
    // cumulative cells (a shared query weighs every reference by the same factor: the reference lengths alone decide)
    std::vector<double> cum((size_t)n + 1);
    cum[0] = 0;
    for (int64_t k = 0; k < n; ++k) {
        const double ql = qoff ? (double)(qoff[k + 1] - qoff[k]) : 1.0;
        cum[k + 1] = cum[k] + ql * (double)(roff[k + 1] - roff[k]);
    }
    bounds[0] = 0;
    for (int g = 1; g < parts; ++g) {
        const double target = cum[n] * (double)g / (double)parts;
        int64_t k = (int64_t)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
        if (k < bounds[g - 1]) k = bounds[g - 1];
        if (k > n) k = n;
        bounds[g] = k;
    }
    bounds[parts] = n;
    return 0;
}

namespace {
struct ShardJob {
    const pmx_config_t *cfg; const parasail_profile_t *profile;
    int64_t lo, hi;
    const uint8_t *qbuf; const int64_t *qoff; const uint8_t *rbuf; const int64_t *roff;
    pmx_record_t *out; pmx_stats_t *stats;
    int device, rc; char err[256];
};
// One persistent host thread per shard slot: its thread-local device scratch, streams and staging survive between calls.
struct ShardWorker {
    std::thread th; std::mutex mx; std::condition_variable cv;
    ShardJob *job = nullptr; bool done = true;
    void loop()
    {
        for (;;) {
            ShardJob *j;
            { std::unique_lock<std::mutex> lk(mx); cv.wait(lk, [&] { return job != nullptr; }); j = job; }
            run(*j);
            { std::lock_guard<std::mutex> lk(mx); job = nullptr; done = true; }
            cv.notify_all();
        }
    }
    static void run(ShardJob &j)
    {
        j.rc = 0; j.err[0] = 0;
        if (hipSetDevice(j.device) != hipSuccess) { j.rc = -1; snprintf(j.err, sizeof j.err, "hipSetDevice(%d) failed", j.device); return; }
        const int64_t m = j.hi - j.lo;
        if (m <= 0) return;
        std::vector<int64_t> ro((size_t)m + 1), qo;
        for (int64_t k = 0; k <= m; ++k) ro[k] = j.roff[j.lo + k] - j.roff[j.lo];
        if (j.profile) {
            j.rc = pmx_align_profile_batch(j.cfg, j.profile, m, j.rbuf + j.roff[j.lo], ro.data(), j.out + j.lo, j.stats ? j.stats + j.lo : nullptr);
        } else {
            qo.resize((size_t)m + 1);
            for (int64_t k = 0; k <= m; ++k) qo[k] = j.qoff[j.lo + k] - j.qoff[j.lo];
            j.rc = pmx_align_batch(j.cfg, m, j.qbuf + j.qoff[j.lo], qo.data(), j.rbuf + j.roff[j.lo], ro.data(), j.out + j.lo,
                                   j.stats ? j.stats + j.lo : nullptr);
        }
        if (j.rc) snprintf(j.err, sizeof j.err, "device %d: %s", j.device, pmx_last_error());
    }
};
std::mutex g_pool_mx;
std::vector<ShardWorker *> g_pool;
}  // namespace

static int multi_run(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                     const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                     const int *devices, int ndev, pmx_record_t *out, pmx_stats_t *stats_out)
{
    if (check_cfg(cfg)) return -1;
    if (n <= 0) return 0;
    if (!devices || ndev <= 0 || ndev > 64) { set_err("bad device list"); return -1; }
    if (!rbuf || !roff || !out || (!profile && (!qbuf || !qoff))) { set_err("null buffer"); return -1; }
    if ((cfg->want & PMX_WANT_STATS) && !stats_out) { set_err("stats requested without a stats buffer"); return -1; }
    const int have = pmx_device_count();
    for (int g = 0; g < ndev; ++g) if (devices[g] < 0 || devices[g] >= have) { set_err("device %d of the list does not exist (%d visible)", devices[g], have); return -1; }
    std::vector<int64_t> bounds((size_t)ndev + 1);
    if (pmx_shard_bounds_by_cells(n, profile ? nullptr : qoff, roff, ndev, bounds.data())) { set_err("shard planner failed"); return -1; }
    std::lock_guard<std::mutex> call_lock(g_pool_mx);          // one multi-GPU call at a time per process (the workers are shared)
    while ((int)g_pool.size() < ndev) {
        ShardWorker *w = new ShardWorker;
        try { w->th = std::thread([w] { w->loop(); }); }
        catch (const std::system_error &e) { delete w; set_err("cannot start a host thread for shard %d: %s", (int)g_pool.size(), e.what()); return -1; }
        w->th.detach();
        g_pool.push_back(w);
    }
    std::vector<ShardJob> jobs((size_t)ndev);
    for (int g = 0; g < ndev; ++g) {
        ShardJob &j = jobs[g];
        j.cfg = cfg; j.profile = profile; j.lo = bounds[g]; j.hi = bounds[g + 1];
        j.qbuf = qbuf; j.qoff = qoff; j.rbuf = rbuf; j.roff = roff; j.out = out; j.stats = stats_out; j.device = devices[g]; j.rc = 0; j.err[0] = 0;
        ShardWorker *w = g_pool[g];
        { std::lock_guard<std::mutex> lk(w->mx); w->job = &j; w->done = false; }
        w->cv.notify_all();
    }
    int rc = 0;
    for (int g = 0; g < ndev; ++g) {
        ShardWorker *w = g_pool[g];
        std::unique_lock<std::mutex> lk(w->mx);
        w->cv.wait(lk, [&] { return w->done; });
        if (jobs[g].rc && !rc) { rc = jobs[g].rc; set_err("%s", jobs[g].err); }
    }
    return rc;
}

extern "C" int pmx_align_batch_multi(const pmx_config_t *cfg, int64_t n,
                                     const uint8_t *qbuf, const int64_t *qoff, const uint8_t *rbuf, const int64_t *roff,
                                     const int *devices, int ndev, pmx_record_t *out, pmx_stats_t *stats_out)
{
    if (n > 0 && qoff && roff && (qoff[0] != 0 || roff[0] != 0)) { set_err("offset arrays must start at 0"); return -1; }
    return multi_run(cfg, nullptr, n, qbuf, qoff, rbuf, roff, devices, ndev, out, stats_out);
}

extern "C" int pmx_align_profile_batch_multi(const pmx_config_t *cfg, const parasail_profile_t *profile, int64_t n,
                                             const uint8_t *rbuf, const int64_t *roff,
                                             const int *devices, int ndev, pmx_record_t *out, pmx_stats_t *stats_out)
{
    if (!profile) { set_err("null profile"); return -1; }
    if (cfg && profile->matrix != cfg->matrix) { set_err("profile was built with a different matrix"); return -1; }
    if (n > 0 && roff && roff[0] != 0) { set_err("offset arrays must start at 0"); return -1; }
    return multi_run(cfg, profile, n, nullptr, nullptr, rbuf, roff, devices, ndev, out, stats_out);
}

extern "C" void pmx_free(void *p) { if (p && !g_text_pool.give_back(p)) free(p); }

// Page-locks a caller-owned host buffer (hipHostRegister) so that the host-buffer batch entries copy it by DMA at full PCIe rate
// instead of through the driver's pageable staging (measured: 39 -> ~55 GB/s); one-time cost, undone by pmx_host_unregister.
extern "C" int pmx_host_register(void *p, size_t bytes)
{
    if (!p || !bytes) return 0;
    HIP_OR_RET(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return 0;
}
extern "C" int pmx_host_unregister(void *p)
{
    if (!p) return 0;
    HIP_OR_RET(hipHostUnregister(p));
    return 0;
}

// ---- sequence-set batches (semantics: include/parasail_amd.h; kernels: pmx_pairs.hip) ----------------------------------
// A set: packed sequences on one device and, for an uploaded set, the host's copy of the offsets (validation, exact maxima).
struct pmx_seqset {
    const uint8_t *d_buf = nullptr; const int64_t *d_off = nullptr;
    int64_t count = 0, bytes = 0;
    int dev = -1;                    // -1: wrapped while no device was usable; every entry refuses such a set
    bool owned = false;
    std::vector<int64_t> h_off;      // count + 1 entries; empty: a wrapped set
};

extern "C" pmx_seqset_t *pmx_seqset_create(const uint8_t *buf, const int64_t *off, int64_t count)
{
    if (!off || count < 0 || (count > 0 && !buf)) { set_err("null buffer or negative count"); return nullptr; }
    if (off[0] < 0) { set_err("offsets must not be negative"); return nullptr; }
    for (int64_t k = 0; k < count; ++k)
        if (off[k + 1] < off[k]) { set_err("offsets decrease at sequence %lld", (long long)k); return nullptr; }
    if (off[count] > ((int64_t)1 << 40)) { set_err("bad offset array"); return nullptr; }
    pmx_seqset *s = new (std::nothrow) pmx_seqset();
    if (!s) { set_err("out of memory"); return nullptr; }
    try { s->h_off.assign(off, off + count + 1); } catch (const std::bad_alloc &) { delete s; set_err("out of memory"); return nullptr; }
    s->count = count; s->bytes = off[count]; s->owned = true;
    void *db = nullptr, *dof = nullptr;
    hipError_t e = hipGetDevice(&s->dev);
    if (e == hipSuccess) e = hipMalloc(&db, (size_t)s->bytes + 16);
    if (e == hipSuccess) e = hipMalloc(&dof, sizeof(int64_t) * (size_t)(count + 1));
    if (e == hipSuccess && s->bytes > 0) e = hipMemcpy(db, buf, (size_t)s->bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dof, off, sizeof(int64_t) * (size_t)(count + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_err("sequence set upload failed: %s", hipGetErrorString(e));
        if (db) (void)hipFree(db);
        if (dof) (void)hipFree(dof);
        delete s; return nullptr;
    }
    s->d_buf = (const uint8_t *)db; s->d_off = (const int64_t *)dof;
    return s;
}

extern "C" pmx_seqset_t *pmx_seqset_wrap_device(const uint8_t *d_buf, const int64_t *d_off, int64_t count, int64_t bytes)
{
    if (!d_off || count < 0 || bytes < 0 || (bytes > 0 && !d_buf)) { set_err("null buffer, negative count or negative bytes"); return nullptr; }
    pmx_seqset *s = new (std::nothrow) pmx_seqset();
    if (!s) { set_err("out of memory"); return nullptr; }
    s->d_buf = d_buf; s->d_off = d_off; s->count = count; s->bytes = bytes;
    if (hipGetDevice(&s->dev) != hipSuccess) s->dev = -1;
    return s;
}

extern "C" void pmx_seqset_free(pmx_seqset_t *s)
{
    if (!s) return;
    if (s->owned) {
        int dev = -1;
        const bool move = hipGetDevice(&dev) == hipSuccess && dev != s->dev;
        if (move) (void)hipSetDevice(s->dev);
        (void)hipFree((void *)s->d_buf); (void)hipFree((void *)s->d_off);
        if (move) (void)hipSetDevice(dev);
    }
    delete s;
}

extern "C" int64_t pmx_seqset_count(const pmx_seqset_t *s) { return s ? s->count : -1; }

extern "C" int64_t pmx_all_pairs_count(int64_t nseq)
{
    if (nseq < 0 || nseq > INT32_MAX) { set_err("nseq %lld is outside 0 .. 2^31 - 1", (long long)nseq); return -1; }
    return nseq * (nseq - 1) / 2;
}

extern "C" int pmx_all_pairs_index(int64_t nseq, int64_t p, int64_t *i, int64_t *j)
{
    const int64_t total = pmx_all_pairs_count(nseq);
    if (total < 0) return -1;
    if (!i || !j) { set_err("null output"); return -1; }
    if (p < 0 || p >= total) { set_err("pair %lld is outside 0 .. %lld", (long long)p, (long long)total - 1); return -1; }
    unsigned long long ui = 0, uj = 0;
    pmx_all_pairs_index_host((unsigned long long)nseq, (unsigned long long)p, &ui, &uj);
    *i = (int64_t)ui; *j = (int64_t)uj;
    return 0;
}

// The prep stream and the events of the chunk pipeline, per thread and device (the pattern of TraceWs).
struct PairsWs { hipStream_t prep = nullptr; hipEvent_t start = nullptr, packed[2] = {nullptr, nullptr}, aligned[2] = {nullptr, nullptr}; int dev = -1; };
static thread_local PairsWs g_pws;
static int pairs_ws_init()
{
    int dev = 0; HIP_OR_RET(hipGetDevice(&dev));
    if (g_pws.dev == dev) return 0;
    if (g_pws.prep) {                                   // the thread moved to another device: release the old device's objects
        (void)hipStreamDestroy(g_pws.prep); (void)hipEventDestroy(g_pws.start);
        for (int k = 0; k < 2; ++k) { (void)hipEventDestroy(g_pws.packed[k]); (void)hipEventDestroy(g_pws.aligned[k]); }
        g_pws = PairsWs();
    }
    HIP_OR_RET(hipStreamCreateWithFlags(&g_pws.prep, hipStreamNonBlocking));
    HIP_OR_RET(hipEventCreateWithFlags(&g_pws.start, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) {
        HIP_OR_RET(hipEventCreateWithFlags(&g_pws.packed[k], hipEventDisableTiming));
        HIP_OR_RET(hipEventCreateWithFlags(&g_pws.aligned[k], hipEventDisableTiming));
    }
    g_pws.dev = dev;
    return 0;
}

// Pairs per chunk.  One chunk's packed windows take at most chunk * (max_qlen + max_rlen + 16) bytes; the default keeps that under
// PMX_PAIRS_CHUNK_BYTES per set of buffers (two sets) and cuts the batch into equal chunks, whole groups of 64 pairs.  256 MiB: a
// million 150 x 150 pairs (316 MB by this bound) are two chunks.  Measured there: one, two and four chunks take
// 3.09, 3.09 and 3.13 ms -- the six launches a chunk adds cost more than the overlap returns, so chunks are as large as the scratch
// allows, and 2 x 256 MiB is small beside the HBM of the cards this runs on.
static const double PMX_PAIRS_CHUNK_BYTES = 256.0 * 1024 * 1024;
// per: alignment slots per logical pair (2 in PMX_STRAND_BOTH, where the buffers hold every pair twice: half as many pairs by default).
static int64_t pairs_chunk(int64_t n, int32_t max_qlen, int32_t max_rlen, const pmx_pairs_opts_t *opts, int per = 1)
{
    if (opts && opts->chunk_pairs > 0) return opts->chunk_pairs < n ? opts->chunk_pairs : n;
    int64_t chunk = (int64_t)(PMX_PAIRS_CHUNK_BYTES / ((double)per * ((double)max_qlen + (double)max_rlen + 16.0)));
    if (chunk < 1) chunk = 1;
    if (chunk >= n) return n;
    const int64_t nchunks = (n + chunk - 1) / chunk;
    chunk = ((n + nchunks - 1) / nchunks + 63) / 64 * 64;
    return chunk > n ? n : chunk;
}

// Everything a set batch refuses before any GPU work, shared by the entries (R == Q for the all-pairs entries).
static int pairs_check(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, const pmx_pairs_opts_t *opts,
                       int32_t max_qlen, int32_t max_rlen, bool stats_buffer, bool ex = false /* pmx_align_pairs_ex[_device]: CIGAR is taken */)
{
    if (check_cfg(cfg)) return -1;
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if ((cfg->want & PMX_WANT_CIGAR) && !ex) { set_err("this set-batch entry has no CIGAR output: pmx_align_pairs_ex[_device] has"); return -1; }
    if ((cfg->want & PMX_WANT_STATS) && !stats_buffer) { set_err("stats requested without a stats buffer"); return -1; }
    if (max_qlen < 1 || max_rlen < 1) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    if (pssm_batch_check(cfg->matrix, max_qlen, max_qlen)) return -1;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (Q->dev != dev || R->dev != dev) {
        set_err("a sequence set of device %d cannot be used on the current device %d", Q->dev != dev ? Q->dev : R->dev, dev); return -1;
    }
    return 0;
}

// The pair materialiser and the chunk loop.  Chunk c: (enumerate,) resolve, two offset scans and the gather on `prep` into buffer set
// c & 1, then -- behind packed[c & 1] -- body(c0, cn, buffers), the chunk's alignment, on the caller's stream, in chunk order: the
// alignment roads keep per-thread scratch (the CIGAR road internal streams too) and never run twice at once.  aligned[c & 1] lets chunk
// c + 2's gather overwrite the set.  Everything `prep` does is waited for by `st`, so `st` ends behind the last body and behind `prep`.
// One chunk: all on `st`.  shape PMX_PAIRS_TRIANGLE / PMX_PAIRS_RECT: pairs [first, first + n) of the upper triangle of Q x Q / of the
// rectangle Q x R, generated per chunk; the body finds the chunk's descriptors, listed or generated, in PairsChunkBufs::pairs.
// What a chunk's cn pairs become is the run's SlotPlan: per alignment slots per pair, so the buffers hold per * cn windows; the body
// still gets c0 and cn in logical pairs.  max_qlen / max_rlen bound what the buffers hold: on a translated side the letters.
enum { TR_NONE = 0, TR_QUERY = 1, TR_REF = 2, TR_CODONS = 3, TR_CODONS_REF = 4 };      // which side an entry translates (the search and top-K entries' `translated`); TR_CODONS: the _frameshift entries, TR_CODONS_REF: the _frameshift_ref entries
struct PairsChunkBufs { uint8_t *q, *r; int32_t *qlen, *rlen; int64_t *qoff, *roff, *qsrc, *rsrc; uint8_t *ok, *sflag; const pmx_pair_t *pairs; int32_t *tw /* the translated side's W */; };
struct SlotPlan;
static int swfs_chunk(const pmx_config_t *cfg, const SlotPlan &plan, int64_t slots, const PairsChunkBufs &b, int32_t max_qlen, int32_t max_rlen,
                      pmx_record_t *d_out, hipStream_t st);

// What the alignment slots of a run's pairs are -- the one place that knows, and the one place a new kind of slot is added: how a pair
// resolves to slots, how a slot's windows reach the chunk buffers, which kernel aligns the slots and how the winner is marked.
//   PLAIN     one slot, the pair as stored: the forward-only kernels, and a forward batch pays nothing for the other kinds' existence.
//   BYTES     one slot on the strand of the pair's byte (the _ex entries, pmx_gather_pairs_device; d_byte NULL: all forward): the
//             gather that can reverse-complement a query window.
//   STRANDS   the strand chosen by the entry: PMX_STRAND_REVERSE one slot, reverse-complemented; PMX_STRAND_BOTH slot 2 k
//             pair k as stored, slot 2 k + 1 with its query reverse-complemented.  The slots fold, the strand is the mark.
//   FRAMES    a translated side (DESIGN 2.5i the query; ref, 2.5j: the reference): that side's windows are nucleotides translated on
//             their way into the buffers, one slot per frame first .. first + per - 1 (1, 3 or 6), or d_byte's frame per pair.  The
//             frame is the mark.
//   CODONS    codon streams (DESIGN 2.5k the query's, aligned by pmx_swfs; ref, 2.5m: the reference's, by pmx_swfsc) of W - 2 letters,
//             one slot per strand first .. first + per - 1, or d_byte's strand per pair, with this frameshift penalty.
struct SlotPlan {
    enum Kind { PLAIN, BYTES, STRANDS, FRAMES, CODONS };
    Kind kind = PLAIN;
    bool ref = false;                       // FRAMES, CODONS: the translated side is the reference's
    int first = 0, per = 1;                 // the slots' flag bytes first .. first + per - 1 for every pair ...
    const uint8_t *d_byte = nullptr;        // ... or (listed pairs, per 1) a byte per pair
    PmxCodeTable code; int frameshift = 0;
    const PmxFsSide &side() const { return pmx_fs_side(ref); }              // CODONS: the sweep of the plan's side
    SlotPlan() {}
    explicit SlotPlan(const uint8_t *d_strand) : kind(d_strand ? BYTES : PLAIN), d_byte(d_strand) {}       // the _ex entries: BYTES where there are strand bytes
    void strands(int strand_mode) { kind = STRANDS; first = strand_mode == PMX_STRAND_REVERSE ? 1 : 0; per = strand_mode == PMX_STRAND_BOTH ? 2 : 1; }
    void set_code(const uint8_t *c) { if (c) memcpy(code.v, c, 64); else pmx_genetic_code_host(code.v); }
    bool translates() const { return kind == FRAMES || kind == CODONS; }
    bool folds() const { return kind >= STRANDS; }                          // the slots' records go through the fold
    int marked() const { return kind == FRAMES ? 2 : folds() ? 1 : 0; }     // what folded records carry in their flags (fold, append_hits, emit): a frame, a strand
    int min_off() const { return per == 1 && !d_byte ? first % 3 : 0; }     // the smallest offset a frame of the call reads from
    // the longest translation of w nucleotides
    int32_t letters(int32_t w) const { return std::max<int32_t>(1, kind == CODONS ? w - 2 : (w - min_off()) / 3); }
    // the maxima in letters (mnr: the shortest reference, or NULL)
    void to_letters(int32_t *mq, int32_t *mr, int32_t *mnr = nullptr) const
    {
        if (!translates()) return;
        if (!ref) { *mq = letters(*mq); return; }
        *mr = letters(*mr);
        if (mnr) *mnr = letters(*mnr);
    }
    // cn descriptors at pc (pairs c0 .. of the run) -> per * cn slots in b's columns
    int resolve(const pmx_pair_t *pc, int64_t c0, int64_t cn, const pmx_seqset *Q, const pmx_seqset *R, int32_t max_qlen, int32_t max_rlen,
                const PairsChunkBufs &b, hipStream_t st) const
    {
        const uint8_t *byte = d_byte ? d_byte + c0 : nullptr;
        switch (kind) {
        case FRAMES:
            return pmx_launch_pairs_resolve_frames(pc, byte, first, per, cn, Q->d_off, Q->count, Q->bytes, R->d_off, R->count, R->bytes, max_qlen, max_rlen,
                                                   b.qlen, b.rlen, b.tw, b.qsrc, b.rsrc, b.ok, b.sflag, st, ref);
        case CODONS:
            return pmx_launch_pairs_resolve_codons(pc, byte, first, per, cn, Q->d_off, Q->count, Q->bytes, R->d_off, R->count, R->bytes, max_qlen, max_rlen,
                                                   b.qlen, b.rlen, b.tw, b.qsrc, b.rsrc, b.ok, b.sflag, st, ref);
        default:
            return pmx_launch_pairs_resolve(pc, byte, first, per, cn, Q->d_off, Q->count, Q->bytes, R->d_off, R->count, R->bytes, max_qlen, max_rlen,
                                            b.qlen, b.rlen, b.qsrc, b.rsrc, b.ok, b.sflag, st);
        }
    }
    // the sn slots' windows into b.q / b.r at b.qoff / b.roff; a window whose end would cross its capacity is not written
    int gather(int64_t sn, const pmx_seqset *Q, const pmx_seqset *R, const PairsChunkBufs &b, int64_t q_cap, int64_t r_cap, hipStream_t st) const
    {
        switch (kind) {
        case PLAIN:
            return pmx_launch_pairs_gather(sn, Q->d_buf, Q->bytes, R->d_buf, R->bytes, b.qlen, b.rlen, b.qsrc, b.rsrc, b.ok, b.qoff, b.roff, b.q, b.r, st);
        case FRAMES:
            return pmx_launch_pairs_gather_translated(sn, Q->d_buf, Q->bytes, R->d_buf, R->bytes, b.qlen, b.rlen, b.tw, b.qsrc, b.rsrc, b.ok,
                                                      b.sflag, b.qoff, b.roff, b.q, q_cap, b.r, r_cap, code, st, ref);
        case CODONS:
            return pmx_launch_pairs_gather_codons(sn, Q->d_buf, Q->bytes, R->d_buf, R->bytes, b.qlen, b.rlen, b.tw, b.qsrc, b.rsrc, b.ok,
                                                  b.sflag, b.qoff, b.roff, b.q, q_cap, b.r, r_cap, code, st, ref);
        default:
            return pmx_launch_pairs_gather_stranded(sn, Q->d_buf, Q->bytes, R->d_buf, R->bytes, b.qlen, b.rlen, b.qsrc, b.rsrc, b.ok,
                                                    b.sflag, b.qoff, b.roff, b.q, q_cap, b.r, r_cap, st);
        }
    }
    // the sn slots of b aligned into rec (and stats); the error is set
    int align(const pmx_config_t *cfg, int64_t sn, const PairsChunkBufs &b, int32_t max_qlen, int32_t max_rlen, pmx_record_t *rec, pmx_stats_t *stats,
              hipStream_t st) const
    {
        if (kind == CODONS) return swfs_chunk(cfg, *this, sn, b, max_qlen, max_rlen, rec, st);
        return run_batch_device(cfg, sn, b.q, b.qoff, 0, b.r, b.roff, max_qlen, max_rlen, rec, stats, st);
    }
    // the per * cn slot records (and statistics) -> cn records, statistics, winners' bytes and validity bytes (each optional); mark: the
    // winner's byte also rides in the record, as marked() says
    int fold(const PairsChunkBufs &b, int64_t cn, bool mark, const pmx_record_t *srec, const pmx_stats_t *sst, pmx_record_t *rec, pmx_stats_t *stats,
             uint8_t *byte_out, uint8_t *okf, hipStream_t st) const
    {
        return pmx_launch_pairs_fold(srec, sst, b.ok, b.sflag, cn, per, mark ? marked() : 0, rec, stats, byte_out, okf, st);
    }
};
template <typename Body>
static int pairs_run(const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs, int64_t first, int shape,
                     const SlotPlan &plan, int32_t max_qlen, int32_t max_rlen, hipStream_t st, int64_t chunk, Body body)
{
    const bool two = chunk < n;
    const int per = plan.per;
    const size_t slots = (size_t)chunk * (size_t)per;
    PairsChunkBufs B[2]; void *scan = nullptr; pmx_pair_t *gen = nullptr;
    const size_t scan_bytes = pmx_text_scan_scratch_bytes((int64_t)slots);
    if (scratch_carve(SCR_PAIRS, [&](Carver &c) {
            for (int s = 0; s < (two ? 2 : 1); ++s) {
                B[s].q = c.take<uint8_t>(slots * (size_t)max_qlen + 16);      // (the slack of the host entries' staged copies)
                B[s].r = c.take<uint8_t>(slots * (size_t)max_rlen + 16);
                B[s].qlen = c.take<int32_t>(slots + 2); B[s].rlen = c.take<int32_t>(slots + 2);
                B[s].qoff = c.take<int64_t>(slots + 1); B[s].roff = c.take<int64_t>(slots + 1);
                B[s].qsrc = c.take<int64_t>(slots); B[s].rsrc = c.take<int64_t>(slots);
                B[s].ok = c.take<uint8_t>(slots);
                B[s].sflag = plan.kind != SlotPlan::PLAIN ? c.take<uint8_t>(slots) : nullptr;
                B[s].tw = plan.translates() ? c.take<int32_t>(slots) : nullptr;
            }
            scan = c.take<unsigned char>(scan_bytes);           // (one: the scans of all chunks run in order on one stream)
        })) return -1;
    const bool listed = shape == PMX_PAIRS_LIST;
    if (!listed && scratch_reserve(sizeof(pmx_pair_t) * (size_t)chunk * (two ? 2 : 1), (void **)&gen, SCR_PGEN)) return -1;
    hipStream_t prep = st;
    if (two) {
        if (pairs_ws_init()) return -1;
        prep = g_pws.prep;
        HIP_OR_RET(hipEventRecord(g_pws.start, st));
        HIP_OR_RET(hipStreamWaitEvent(prep, g_pws.start, 0));
    }
    auto pack = [&](int64_t c0, int64_t cn, int slot) -> int {
        pmx_pair_t *gc = gen ? gen + (size_t)slot * (size_t)chunk : nullptr;
        const pmx_pair_t *pc = listed ? d_pairs + c0 : gc;
        B[slot].pairs = pc;
        const PairsChunkBufs &b = B[slot];
        int rc = listed ? 0 : shape == PMX_PAIRS_TRIANGLE ? pmx_launch_all_pairs_enumerate(Q->count, first + c0, cn, gc, prep)
                                                          : pmx_launch_rect_pairs_enumerate(R->count, first + c0, cn, gc, prep);
        const int64_t sn = cn * per;                              // the chunk's alignment slots
        if (!rc) rc = plan.resolve(pc, c0, cn, Q, R, max_qlen, max_rlen, b, prep);
        if (!rc) rc = pmx_launch_text_offsets(b.qlen, sn, b.qoff, scan, scan_bytes, prep);
        if (!rc) rc = pmx_launch_text_offsets(b.rlen, sn, b.roff, scan, scan_bytes, prep);
        if (!rc) rc = plan.gather(sn, Q, R, b, INT64_MAX, INT64_MAX, prep);
        if (rc) { set_err("pair materialisation failed (%d)", rc); return rc; }
        if (two) HIP_OR_RET(hipEventRecord(g_pws.packed[slot], prep));
        return 0;
    };
    int rc = pack(0, chunk, 0);
    if (rc) return rc;
    int idx = 0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk, ++idx) {
        const int slot = idx & 1;
        const int64_t cn = n - c0 < chunk ? n - c0 : chunk, n0 = c0 + chunk;
        if (n0 < n) {                                                                   // the next chunk's windows, beside this alignment
            if (idx >= 1) HIP_OR_RET(hipStreamWaitEvent(prep, g_pws.aligned[slot ^ 1], 0));      // that set's last alignment is done
            rc = pack(n0, n - n0 < chunk ? n - n0 : chunk, slot ^ 1);
            if (rc) return rc;
        }
        if (two) HIP_OR_RET(hipStreamWaitEvent(st, g_pws.packed[slot], 0));
        rc = body(c0, cn, B[two ? slot : 0]);
        if (rc) return rc;
        if (two) HIP_OR_RET(hipEventRecord(g_pws.aligned[slot], st));
    }
    return 0;
}

// A run of several slots per pair reports which one won: refused where that output is `wanted` and missing.
static int byte_out_check(const SlotPlan &plan, bool wanted, const void *byte_out)
{
    if (!wanted || plan.per < 2 || byte_out) return 0;
    set_err(plan.kind == SlotPlan::FRAMES ? "null frame output: a multi-frame mode reports which frame won" : "null strand output: both strands report which one won");
    return -1;
}
// What every entry over listed pairs, device or host, refuses first, in this order.  both (pmx_align_pairs_both[_device], whose plan is
// known before its configuration is looked at): the strand output, checked ahead of the options.
static int listed_entry_check(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const void *pairs, const void *out,
                              const pmx_pairs_opts_t *opts, const SlotPlan *both = nullptr, const void *strand_out = nullptr)
{
    if (!Q || !R) { set_err("null sequence set"); return -1; }
    if (n < 0) { set_err("negative n"); return -1; }
    if (n > 0 && (!pairs || !out)) { set_err("null pairs or records"); return -1; }
    if (both && byte_out_check(*both, n > 0, strand_out)) return -1;
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    return check_cfg(cfg);
}

// The score road of a set batch of one slot per pair that needs no fold (PLAIN, BYTES): every chunk through run_batch_device, then the
// records (and statistics) of its bad pairs.
static int pairs_run_scores(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs, int64_t first,
                            const SlotPlan &plan, int32_t max_qlen, int32_t max_rlen,
                            pmx_record_t *d_out, pmx_stats_t *d_stats_out, hipStream_t st, int64_t chunk)
{
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    return pairs_run(Q, R, n, d_pairs, first, d_pairs ? PMX_PAIRS_LIST : PMX_PAIRS_TRIANGLE, plan, max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            int rc = plan.align(cfg, cn, b, max_qlen, max_rlen, d_out + c0, stats ? d_stats_out + c0 : nullptr, st);
            if (rc) return rc;
            rc = pmx_launch_pairs_fixup(b.ok, cn, d_out + c0, stats ? d_stats_out + c0 : nullptr, st);
            if (rc) { set_err("bad-pair fix-up launch failed (%d)", rc); return rc; }
            return 0;
        });
}

// The score road of a set batch over listed pairs whose slots fold (STRANDS, FRAMES, CODONS): every chunk's per * cn slots aligned into
// scratch, then the fold straight into the caller's arrays (it writes the bad pairs' records too; per 1: the one slot's record and byte).
static int pairs_run_folded(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs,
                            const SlotPlan &plan, int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_byte_out,
                            hipStream_t st, int64_t chunk)
{
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    pmx_record_t *srec = nullptr; pmx_stats_t *sst = nullptr;
    if (scratch_carve(SCR_PSRCH, [&](Carver &c) {
            srec = c.take<pmx_record_t>((size_t)plan.per * (size_t)chunk);
            sst = stats ? c.take<pmx_stats_t>((size_t)plan.per * (size_t)chunk) : nullptr;
        })) return -1;
    return pairs_run(Q, R, n, d_pairs, 0, PMX_PAIRS_LIST, plan, max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            int rc = plan.align(cfg, plan.per * cn, b, max_qlen, max_rlen, srec, sst, st);
            if (rc) return rc;
            rc = plan.fold(b, cn, false, srec, sst, d_out + c0, stats ? d_stats_out + c0 : nullptr, d_byte_out ? d_byte_out + c0 : nullptr, nullptr, st);
            if (rc) set_err("%s fold launch failed (%d)", plan.kind == SlotPlan::FRAMES ? "frame" : "strand", rc);
            return rc;
        });
}

extern "C" int pmx_align_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                      int64_t n, const pmx_pair_t *d_pairs, int32_t max_qlen, int32_t max_rlen,
                                      pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream, const pmx_pairs_opts_t *opts)
{
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts)) return -1;
    if (n == 0) return 0;
    if (pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats_out != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_scores(cfg, Q, R, n, d_pairs, 0, SlotPlan(), max_qlen, max_rlen, d_out, d_stats_out, (hipStream_t)stream, pairs_chunk(n, max_qlen, max_rlen, opts));
}

// ---- the strand chosen by the entry ----
// What every entry with a strand mode refuses about it, before any GPU work.  *plan: a mode other than PMX_STRAND_FORWARD makes the run's
// slots the strands (forward leaves the plan what it is: PLAIN, or what side_check made of it).
static int strand_mode_check(const pmx_config_t *cfg, int strand_mode, SlotPlan *plan)
{
    if (strand_mode < PMX_STRAND_FORWARD || strand_mode > PMX_STRAND_BOTH) {
        set_err("strand mode %d is outside 0 .. 2 (PMX_STRAND_FORWARD, PMX_STRAND_REVERSE, PMX_STRAND_BOTH)", strand_mode); return -1;
    }
    if (strand_mode != PMX_STRAND_FORWARD && cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {
        set_err("a strand mode other than PMX_STRAND_FORWARD takes no PSSM matrix: a reversed query has no PSSM"); return -1;
    }
    if (strand_mode != PMX_STRAND_FORWARD) plan->strands(strand_mode);
    return 0;
}
static int pairs_both_want_check(const pmx_config_t *cfg)
{
    if (cfg->want & PMX_WANT_CIGAR) {
        set_err("pmx_align_pairs_both[_device] has no CIGAR output: pass the returned strand bytes to pmx_align_pairs_ex[_device] with PMX_WANT_CIGAR");
        return -1;
    }
    return 0;
}

extern "C" int pmx_align_pairs_both_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                           int64_t n, const pmx_pair_t *d_pairs, int32_t max_qlen, int32_t max_rlen,
                                           pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_strand_out, void *stream,
                                           const pmx_pairs_opts_t *opts)
{
    SlotPlan plan;
    plan.strands(PMX_STRAND_BOTH);
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts, &plan, d_strand_out) || pairs_both_want_check(cfg) ||
        strand_mode_check(cfg, PMX_STRAND_BOTH, &plan)) return -1;
    if (n == 0) return 0;
    if (pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats_out != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_folded(cfg, Q, R, n, d_pairs, plan, max_qlen, max_rlen, d_out, d_stats_out, d_strand_out, (hipStream_t)stream,
                            pairs_chunk(n, max_qlen, max_rlen, opts, plan.per));
}

// ---- a translated side: the query's or the reference's (2.5j) ----
extern "C" void pmx_genetic_code_table(uint8_t table[64]) { if (table) pmx_genetic_code_host(table); }

// What every translated entry refuses about its frames, matrix and outputs, before any GPU work.  *fr: the run's frames, code and side
// (ref: the _translated_ref entries).
static int frames_check(const pmx_config_t *cfg, int frame_mode, const uint8_t *d_frame, const uint8_t *code, SlotPlan *fr, bool ref = false)
{
    if (frame_mode < 0 || frame_mode > PMX_FRAMES_ALL) {
        set_err("frame mode %d is outside 0 .. 8 (a frame 0 .. 5, PMX_FRAMES_FORWARD, PMX_FRAMES_REVERSE, PMX_FRAMES_ALL)", frame_mode); return -1;
    }
    if (d_frame && frame_mode != 0) { set_err("a frame byte per pair takes frame mode 0, not %d", frame_mode); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {
        set_err(ref ? "a translated reference takes no PSSM matrix: the profile would belong to the protein query, but the batch PSSM forms are not wired "
                      "through the translated entries"
                    : "a translated query takes no PSSM matrix: a profile belongs to one protein query");
        return -1;
    }
    if (cfg->want & PMX_WANT_CIGAR) {
        set_err("the translated entries have no CIGAR output: pass the pairs and their frame bytes to %s, "
                "then run pmx_align_batch_cigar_device over the packed buffers", ref ? "pmx_gather_pairs_translated_ref_device" : "pmx_gather_pairs_translated_device");
        return -1;
    }
    fr->kind = SlotPlan::FRAMES; fr->ref = ref;
    fr->first = frame_mode <= 5 ? frame_mode : frame_mode == PMX_FRAMES_REVERSE ? 3 : 0;
    fr->per = frame_mode <= 5 ? 1 : frame_mode == PMX_FRAMES_ALL ? 6 : 3;
    fr->d_byte = d_frame;
    fr->set_code(code);
    return 0;
}

// Both device entries over listed pairs: ref false pmx_align_pairs_translated_device, true pmx_align_pairs_translated_ref_device.
static int align_pairs_frames_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                     int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_frame, int frame_mode, const uint8_t *code,
                                     int32_t max_qlen, int32_t max_rlen,
                                     pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_frame_out, void *stream,
                                     const pmx_pairs_opts_t *opts, bool ref)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts) || frames_check(cfg, frame_mode, d_frame, code, &fr, ref) ||
        byte_out_check(fr, n > 0, d_frame_out)) return -1;
    if (n == 0) return 0;
    if (pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats_out != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_folded(cfg, Q, R, n, d_pairs, fr, max_qlen, max_rlen, d_out, d_stats_out, d_frame_out, (hipStream_t)stream,
                            pairs_chunk(n, max_qlen, max_rlen, opts, fr.per));
}

extern "C" int pmx_align_pairs_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                 int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_frame, int frame_mode, const uint8_t *code,
                                                 int32_t max_qlen, int32_t max_rlen,
                                                 pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_frame_out, void *stream,
                                                 const pmx_pairs_opts_t *opts)
{
    return align_pairs_frames_device(cfg, Q, R, n, d_pairs, d_frame, frame_mode, code, max_qlen, max_rlen, d_out, d_stats_out, d_frame_out, stream, opts, false);
}

extern "C" int pmx_align_pairs_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                     int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_frame, int frame_mode, const uint8_t *code,
                                                     int32_t max_qlen, int32_t max_rlen,
                                                     pmx_record_t *d_out, pmx_stats_t *d_stats_out, uint8_t *d_frame_out, void *stream,
                                                     const pmx_pairs_opts_t *opts)
{
    return align_pairs_frames_device(cfg, Q, R, n, d_pairs, d_frame, frame_mode, code, max_qlen, max_rlen, d_out, d_stats_out, d_frame_out, stream, opts, true);
}

// The five gather hooks (pmx_gather_pairs_device: BYTES; _translated[_ref]: FRAMES; _codons[_ref]: CODONS): one slot per pair with the
// pair's byte (d_byte NULL: all 0), resolved, scanned and gathered into the caller's buffers up to their capacities.
static int gather_pairs_hook(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                             SlotPlan::Kind kind, bool ref, const uint8_t *d_byte, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                             uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                             uint8_t *d_ok, void *stream)
{
    if (!Q || !R) { set_err("null sequence set"); return -1; }
    if (n < 0 || q_capacity < 0 || r_capacity < 0) { set_err("negative n or capacity"); return -1; }
    if (!d_qoff || !d_roff || (n > 0 && (!d_pairs || !d_qout || !d_rout))) { set_err("null buffer"); return -1; }
    if (max_qlen < 1 || max_rlen < 1) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    if (n == 0) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (Q->dev != dev || R->dev != dev) {
        set_err("a sequence set of device %d cannot be used on the current device %d", Q->dev != dev ? Q->dev : R->dev, dev); return -1;
    }
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    SlotPlan plan;
    plan.kind = kind; plan.ref = ref; plan.d_byte = d_byte;
    if (plan.translates()) plan.set_code(code);
    PairsChunkBufs b = {d_qout, d_rout, nullptr, nullptr, d_qoff, d_roff, nullptr, nullptr, nullptr, nullptr, d_pairs, nullptr};
    void *scan = nullptr;
    const size_t scan_bytes = pmx_text_scan_scratch_bytes(n);
    if (scratch_carve(SCR_PAIRS, [&](Carver &c) {
            b.qlen = c.take<int32_t>((size_t)n + 2); b.rlen = c.take<int32_t>((size_t)n + 2);
            b.tw = plan.translates() ? c.take<int32_t>((size_t)n) : nullptr;
            b.qsrc = c.take<int64_t>((size_t)n); b.rsrc = c.take<int64_t>((size_t)n);
            b.ok = c.take<uint8_t>((size_t)n); b.sflag = c.take<uint8_t>((size_t)n);
            scan = c.take<unsigned char>(scan_bytes);
        })) return -1;
    if (d_ok) b.ok = d_ok;
    int rc = plan.resolve(d_pairs, 0, n, Q, R, max_qlen, max_rlen, b, st);
    if (!rc) rc = pmx_launch_text_offsets(b.qlen, n, d_qoff, scan, scan_bytes, st);
    if (!rc) rc = pmx_launch_text_offsets(b.rlen, n, d_roff, scan, scan_bytes, st);
    if (!rc) rc = plan.gather(n, Q, R, b, q_capacity, r_capacity, st);
    if (rc) { set_err("pair materialisation failed (%d)", rc); return rc; }
    return 0;
}

extern "C" int pmx_gather_pairs_translated_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                                  const uint8_t *d_frame, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                  uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                                  uint8_t *d_ok, void *stream)
{
    return gather_pairs_hook(Q, R, n, d_pairs, SlotPlan::FRAMES, false, d_frame, code, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream);
}

extern "C" int pmx_gather_pairs_translated_ref_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                                      const uint8_t *d_frame, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                      uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                                      uint8_t *d_ok, void *stream)
{
    return gather_pairs_hook(Q, R, n, d_pairs, SlotPlan::FRAMES, true, d_frame, code, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream);
}

// ---- frameshift-aware translated search: codon streams through pmx_swfs ----
extern "C" int32_t pmx_frameshift_max_window(void) { return PMX_FRAMESHIFT_MAX_WINDOW; }

// What every _frameshift entry refuses about its strand mode, penalty, matrix, mode, width and outputs, before any GPU work.  *fr: the
// run's strands (d_strand: a strand byte per pair, listed pairs only), code and penalty.
static int frameshift_check(const pmx_config_t *cfg, int strand_mode, const uint8_t *d_strand, int32_t frameshift, const uint8_t *code, SlotPlan *fr,
                            bool traceback = false /* the _frameshift_cigar entries: the outputs are theirs to check */,
                            bool ref = false /* the _frameshift_ref entries: the strands and the stream are the reference's */)
{
    if (strand_mode < PMX_STRAND_FORWARD || strand_mode > PMX_STRAND_BOTH) {
        set_err("strand mode %d is outside 0 .. 2 (PMX_STRAND_FORWARD, PMX_STRAND_REVERSE, PMX_STRAND_BOTH)", strand_mode); return -1;
    }
    if (d_strand && strand_mode != PMX_STRAND_FORWARD) { set_err("a strand byte per pair takes strand mode PMX_STRAND_FORWARD, not %d", strand_mode); return -1; }
    if (frameshift < 0) { set_err("the frameshift penalty is passed as a non-negative number, not %d", (int)frameshift); return -1; }
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {
        set_err(ref ? "the reference-side frameshift entries take no PSSM matrix: the profile would belong to the protein query, but the kernel has no PSSM form"
                    : "the frameshift entries take no PSSM matrix: a profile belongs to one protein query");
        return -1;
    }
    if (cfg->mode != PMX_MODE_SW) { set_err("the frameshift entries align locally: mode %d is not PMX_MODE_SW", cfg->mode); return -1; }
    if (cfg->width != 0 && cfg->width != 32) { set_err("the frameshift entries compute in 32 bits: width %d is neither 0 nor 32", cfg->width); return -1; }
    if (!traceback && (cfg->want & PMX_WANT_STATS)) { set_err("the frameshift entries have no statistics (PMX_WANT_STATS)"); return -1; }
    if (!traceback && (cfg->want & PMX_WANT_CIGAR)) {
        set_err(ref ? "the reference-side frameshift entries have no CIGAR output (PMX_WANT_CIGAR): this side has no traceback yet, the hit list is the interface"
                    : "the frameshift entries have no CIGAR output (PMX_WANT_CIGAR): there is no traceback with frameshift operators");
        return -1;
    }
    if (cfg->matrix->size > pmx_fs_side(ref).max_msize) {
        set_err("the frameshift kernel keeps the matrix in LDS: %d symbols exceed %d", cfg->matrix->size, pmx_fs_side(ref).max_msize); return -1;
    }
    fr->strands(strand_mode);                                     // (first and per of the mode; forward: strand 0, one slot)
    fr->kind = SlotPlan::CODONS; fr->ref = ref; fr->frameshift = frameshift;
    fr->d_byte = d_strand;
    fr->set_code(code);
    return 0;
}
// max_qlen bounds N = W - 2, the rows the kernel sees.  ref (the _frameshift_ref entries): max_qlen bounds the protein's letters, the
// rows of pmx_swfsc; the stream on the columns has no cap of its own.
static int frameshift_rows_check(int32_t max_qlen, bool ref = false)
{
    const int max_rows = pmx_fs_side(ref).max_rows;
    if (max_qlen <= max_rows) return 0;
    if (ref) set_err("a query of %d letters exceeds PMX_FRAMESHIFT_REF_MAX_QUERY = %d letters", (int)max_qlen, max_rows);
    else set_err("a codon stream of %d letters exceeds the %d of the longest window, PMX_FRAMESHIFT_MAX_WINDOW = %d nucleotides",
                 (int)max_qlen, max_rows, PMX_FRAMESHIFT_MAX_WINDOW);
    return -1;
}
// The search and top-K entries: the rows' bound of the plan's streams, nothing for the other kinds.
static int codons_rows_check(const SlotPlan &plan, int32_t max_qlen)
{
    return plan.kind == SlotPlan::CODONS ? frameshift_rows_check(max_qlen, plan.ref) : 0;
}

// A chunk's alignment: `slots` codon streams of b against their proteins into d_out.  Streams longer than one strip keep their
// boundary columns in scratch, at most 256 MiB of it: the launcher then runs the slots in parts.  fr.ref: the streams are the
// reference slots and the kernel is pmx_swfsc, whose strips are cut from the protein's rows.
static int swfs_chunk(const pmx_config_t *cfg, const SlotPlan &fr, int64_t slots, const PairsChunkBufs &b, int32_t max_qlen, int32_t max_rlen,
                      pmx_record_t *d_out, hipStream_t st)
{
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    PmxBatch pb = {b.q, b.qoff, b.r, b.roff, slots, max_qlen, max_rlen, 0, nullptr, nullptr, nullptr, 0, 0};
    void *bnd = nullptr; long long bnd_slots = 0;
    const PmxFsSide &side = fr.side();
    if (max_qlen > side.strip_rows) {
        const size_t per_slot = (size_t)side.bound_bytes_per_slot(max_rlen);
        bnd_slots = std::max<long long>(4, (long long)(PMX_PAIRS_CHUNK_BYTES / (double)per_slot) / 4 * 4);
        bnd_slots = std::min<long long>(bnd_slots, (slots + 3) / 4 * 4);
        if (scratch_reserve(per_slot * (size_t)bnd_slots, &bnd, SCR_SWFS)) return -1;
    }
    const int rc = side.launch(pb, dm.d, cfg->open, cfg->extend, fr.frameshift, bnd, bnd_slots, nullptr, d_out, st, &g_last_kernel);
    if (rc) { set_err(rc < 0 ? "frameshift kernel launch failed: %s" : "the frameshift kernel does not take this batch%s", rc < 0 ? hipGetErrorString((hipError_t)(-rc)) : ""); return -1; }
    return 0;
}

// Both device entries over listed pairs: ref false pmx_align_pairs_frameshift_device, true pmx_align_pairs_frameshift_ref_device.
static int align_pairs_codons_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                     int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                     int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                     pmx_record_t *d_out, uint8_t *d_strand_out, void *stream, const pmx_pairs_opts_t *opts, bool ref)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts) || frameshift_check(cfg, strand_mode, d_strand, frameshift, code, &fr, false, ref) ||
        byte_out_check(fr, n > 0, d_strand_out)) return -1;
    if (n == 0) return 0;
    if (frameshift_rows_check(max_qlen, ref) || pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, false)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_folded(cfg, Q, R, n, d_pairs, fr, max_qlen, max_rlen, d_out, nullptr, d_strand_out, (hipStream_t)stream,
                            pairs_chunk(n, max_qlen, max_rlen, opts, fr.per));
}

extern "C" int pmx_align_pairs_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                 int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                 int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                 pmx_record_t *d_out, uint8_t *d_strand_out, void *stream, const pmx_pairs_opts_t *opts)
{
    return align_pairs_codons_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, code, max_qlen, max_rlen, d_out, d_strand_out, stream, opts, false);
}

// ---- frameshift-aware translated search, reference side: the reference windows' codon streams through pmx_swfsc ----
extern "C" int32_t pmx_frameshift_ref_max_query(void) { return PMX_FRAMESHIFT_REF_MAX_QUERY; }

extern "C" int pmx_align_pairs_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                     int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                     int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                     pmx_record_t *d_out, uint8_t *d_strand_out, void *stream, const pmx_pairs_opts_t *opts)
{
    return align_pairs_codons_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, code, max_qlen, max_rlen, d_out, d_strand_out, stream, opts, true);
}

// ---- frameshift traceback: the trace form of pmx_swfs, the walk of pmx_walkfs.hip, the device text rendering ----
// What the _frameshift_cigar entries refuse about their outputs, before any GPU work.  text: d_cigar_text / cigar_buf.
static int frameshift_cigar_outputs_check(const pmx_config_t *cfg, const void *stats, const void *text, int64_t capacity, const void *text_off)
{
    if (!(cfg->want & PMX_WANT_CIGAR)) { set_err("the frameshift traceback entries write CIGAR text: cfg->want must hold PMX_WANT_CIGAR"); return -1; }
    if ((cfg->want & PMX_WANT_STATS) && !stats) { set_err("stats requested without a stats buffer"); return -1; }
    if (!(cfg->want & PMX_WANT_STATS) && stats) { set_err("stats buffer without PMX_WANT_STATS"); return -1; }
    if (!text || !text_off) { set_err("null cigar output"); return -1; }
    if (capacity < 0) { set_err("negative cigar_capacity"); return -1; }
    return 0;
}
// The bound on a chunk's trace scratch: 256 MiB, or what the value switch PMX_CIGAR_CHUNK_BYTES says.  One workgroup of the sweep is
// four slots: a call whose four slots exceed the bound is refused.
static double frameshift_trace_bound()
{
    const char *forced = pmx_env("PMX_CIGAR_CHUNK_BYTES");
    return forced ? atof(forced) : PMX_PAIRS_CHUNK_BYTES;
}
// The trace bytes of one slot: the query side's sweep stores by column, the reference side's by step (pmx_swfs.hip, pmx_swfsc.hip).
static size_t frameshift_trace_bytes_per_slot(bool ref, int32_t max_qlen, int32_t max_rlen)
{
    return (size_t)pmx_fs_side(ref).trace_bytes_per_slot(max_qlen, max_rlen);
}
static int frameshift_trace_bound_check(size_t bytes_per_slot, int32_t max_qlen, int32_t max_rlen)
{
    const double four = 4.0 * (double)bytes_per_slot, bound = frameshift_trace_bound();
    if (four > bound) {
        set_err("four slots of frameshift trace, %.0f bytes at max_qlen %d and max_rlen %d, exceed the bound of %.0f bytes on a chunk's trace "
                "scratch (256 MiB, or PMX_CIGAR_CHUNK_BYTES)", four, (int)max_qlen, (int)max_rlen, bound);
        return -1;
    }
    return 0;
}

// The traceback road of a frameshift batch over listed pairs.  A chunk's per * cn slots run in parts that keep the trace under the
// bound, whole workgroups of four slots: the trace sweep of a part, the strand fold into the caller's arrays (it writes the bad pairs'
// records too), the walk over the winners' traces -- so both slots of a pair keep their trace until the walk -- and the render, all on
// `st`: a part's scratch is free when the next part begins.  The text continues behind the parts and chunks before it
// (d_text_off[c0 + p0], left by the part before on the same stream), so neither chunk_pairs nor the bound changes a byte.
// Scratch: the trace in SCR_TRACE, the op slots in SCR_OPS and the walk's counts in SCR_CIG, which no other road of this call uses.
// fr.side(): the side comes with the plan -- its trace form, strip test and boundary bytes, and the walk's form; the bound, the parts, the fold, the scan, the render and the text rebase are the same code.
static int pairs_run_codons_cigar(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs,
                                  int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats,
                                  int32_t *d_beg, char *d_text, int64_t capacity, int64_t *d_text_off,
                                  hipStream_t st, int64_t chunk, const SlotPlan &fr,
                                  bool continues = false /* the pairs are a later stretch of a longer text: d_text_off[0] holds its total so far */)
{
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    const int per = fr.per;
    const PmxFsSide &side = fr.side();
    const size_t tps = (size_t)side.trace_bytes_per_slot(max_qlen, max_rlen);
    const bool strips = max_qlen > side.strip_rows;
    const size_t bps = (size_t)side.bound_bytes_per_slot(max_rlen);
    int64_t part_slots = (int64_t)(frameshift_trace_bound() / (double)tps) / 4 * 4;           // (at least four: the caller has checked)
    part_slots = std::min<int64_t>(part_slots, ((int64_t)per * chunk + 3) / 4 * 4);
    const int64_t part = part_slots / per;
    void *trace = nullptr, *bnd = nullptr;
    pmx_record_t *srec = nullptr; int64_t *local_off = nullptr, *pair_qoff = nullptr, *pair_roff = nullptr;
    SlotText t;
    // a path has at most N + m ops (matches + reference gaps <= m, 2 matches + 3 codon gaps <= N + 2, frameshift ops <= matches - 1), so
    // the implicit op slot of N + m + 1 entries that pmx_launch_cigar_render_slots assumes per alignment slot holds it
    if (scratch_reserve(tps * (size_t)part_slots, &trace, SCR_TRACE) ||
        (strips && scratch_reserve(bps * (size_t)part_slots, &bnd, SCR_SWFS)) ||
        t.reserve_ops((size_t)part_slots * ((size_t)max_qlen + (size_t)max_rlen + 1)) ||
        scratch_carve(SCR_PSRCH, [&](Carver &c) { srec = c.take<pmx_record_t>((size_t)per * (size_t)chunk); }) ||
        scratch_carve(SCR_CIG, [&](Carver &c) {
            t.carve(c, part);
            local_off = c.take<int64_t>((size_t)part + 1); pair_qoff = c.take<int64_t>((size_t)part + 1); pair_roff = c.take<int64_t>((size_t)part + 1);
        })) return -1;
    return pairs_run(Q, R, n, d_pairs, 0, PMX_PAIRS_LIST, fr, max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            for (int64_t p0 = 0; p0 < cn; p0 += part) {
                const int64_t pn = std::min<int64_t>(part, cn - p0), s0 = per * p0, g0 = c0 + p0;
                const PmxBatch pb = {b.q, b.qoff + s0, b.r, b.roff + s0, per * pn, max_qlen, max_rlen, 0, nullptr, nullptr, nullptr, 0, 0};
                int rc = side.launch_trace(pb, dm.d, cfg->open, cfg->extend, fr.frameshift, bnd, 0, trace, srec + s0, st, &g_last_kernel);
                if (rc) { set_err(rc < 0 ? "frameshift trace kernel launch failed: %s" : "the frameshift trace kernel does not take this batch%s", rc < 0 ? hipGetErrorString((hipError_t)(-rc)) : ""); return -1; }
                uint8_t *won = d_strand_out ? d_strand_out + g0 : nullptr;
                rc = pmx_launch_pairs_fold(srec + s0, nullptr, b.ok + s0, b.sflag + s0, pn, per, 0, d_out + g0, nullptr, won, nullptr, st);
                if (rc) { set_err("strand fold launch failed (%d)", rc); return rc; }
                rc = pmx_launch_walkfs(dm.d, pn, per, per == 2 ? won : nullptr, b.q, b.qoff + s0, b.r, b.roff + s0, max_rlen, d_out + g0,
                                       (const uint8_t *)trace, (long long)tps, t.ops, t.nops, t.textlen, pair_qoff, pair_roff,
                                       d_beg ? d_beg + 2 * g0 : nullptr, d_stats ? d_stats + g0 : nullptr, st, side.ref);
                if (rc) { set_err("frameshift walk launch failed (%d)", rc); return rc < 0 ? rc : -1; }
                rc = t.render(pair_qoff, pair_roff, 0, pn, d_text, capacity, d_text_off + g0, st, g0 > 0 || continues ? local_off : nullptr);
                if (rc) return rc;
            }
            return 0;
        });
}

// Both device traceback entries: ref false pmx_align_pairs_frameshift_cigar_device, true pmx_align_pairs_frameshift_ref_cigar_device.
static int align_pairs_codons_cigar_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                           int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                           int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                           pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats, int32_t *d_beg,
                                           char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off,
                                           void *stream, const pmx_pairs_opts_t *opts, bool ref)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts) || frameshift_check(cfg, strand_mode, d_strand, frameshift, code, &fr, true, ref) ||
        frameshift_cigar_outputs_check(cfg, d_stats, d_cigar_text, cigar_capacity, d_cigar_off) || byte_out_check(fr, n > 0, d_strand_out)) return -1;
    if (n == 0) return 0;
    if (frameshift_rows_check(max_qlen, ref) || frameshift_trace_bound_check(frameshift_trace_bytes_per_slot(ref, max_qlen, max_rlen), max_qlen, max_rlen) ||
        pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats != nullptr, true)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_codons_cigar(cfg, Q, R, n, d_pairs, max_qlen, max_rlen, d_out, d_strand_out, d_stats, d_beg, d_cigar_text, cigar_capacity,
                                  d_cigar_off, (hipStream_t)stream, pairs_chunk(n, max_qlen, max_rlen, opts, fr.per), fr);
}

extern "C" int pmx_align_pairs_frameshift_cigar_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                       int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                       int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                       pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats, int32_t *d_beg,
                                                       char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off,
                                                       void *stream, const pmx_pairs_opts_t *opts)
{
    return align_pairs_codons_cigar_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, code, max_qlen, max_rlen, d_out, d_strand_out,
                                           d_stats, d_beg, d_cigar_text, cigar_capacity, d_cigar_off, stream, opts, false);
}

// ---- frameshift traceback, reference side: the trace form of pmx_swfsc, the <true> form of the walk, the same road ----
extern "C" int pmx_align_pairs_frameshift_ref_cigar_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                           int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                           int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                           pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats, int32_t *d_beg,
                                                           char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off,
                                                           void *stream, const pmx_pairs_opts_t *opts)
{
    return align_pairs_codons_cigar_device(cfg, Q, R, n, d_pairs, d_strand, strand_mode, frameshift, code, max_qlen, max_rlen, d_out, d_strand_out,
                                           d_stats, d_beg, d_cigar_text, cigar_capacity, d_cigar_off, stream, opts, true);
}

// ---- windowed frameshift traceback, reference side: the score road, the window of every record, the trace road over it ----
static thread_local int64_t g_fswin_parts = 0;
extern "C" int64_t pmx_frameshift_ref_cigar_long_parts(void) { return g_fswin_parts; }

// The road of the _frameshift_ref_cigar_long entries.  Per chunk of `chunk` pairs, all on `st`:
//   1. the score road of pmx_align_pairs_frameshift_ref_device over the full windows (both strands swept and folded in
//      PMX_STRAND_BOTH) into scratch: the chunk's records, and the winners' strands;
//   2. pmx_fsref_window_kernel: every record's narrowed descriptor, column shift and narrowed lengths;
//   3. the lengths to the host -- THE ONE SYNCHRONISATION OF `st` PER CHUNK;
//   4. pairs_run_codons_cigar over the narrowed descriptors, one slot per pair on the winner's strand, in parts of consecutive pairs
//      cut greedily so that a part's slots (whole workgroups of four) times the trace of its own narrowed maxima stay under the bound:
//      a weak hit with a wide window shrinks its own part only, and op slots, boundary scratch and trace stride are the part's;
//   5. pmx_fsref_rebase_kernel: end_ref and beg_ref back into the pair's window, and the rebased record held against step 1's.
// A record that differs is a bug in the window's proof, not an input condition: the call returns -1 ("window proof violated"); the count
// is read with the next chunk's lengths and once behind the last chunk.  A pair whose narrowed window alone exceeds the bound with four
// slots is refused behind the score pass of its chunk.  The text continues behind the parts and chunks before it, so neither
// chunk_pairs nor the bound nor the parts change a byte.
static int pairs_run_codons_cigar_windowed(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs,
                                           int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats,
                                           int32_t *d_beg, char *d_text, int64_t capacity, int64_t *d_text_off,
                                           hipStream_t st, int64_t chunk, const SlotPlan &fr)
{
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    pmx_record_t *rec1 = nullptr; pmx_pair_t *npairs = nullptr; int32_t *ashift = nullptr, *nlen = nullptr; uint8_t *sbuf = nullptr; unsigned *viol = nullptr;
    if (scratch_carve(SCR_FSWIN, [&](Carver &c) {
            rec1 = c.take<pmx_record_t>((size_t)chunk); npairs = c.take<pmx_pair_t>((size_t)chunk);
            ashift = c.take<int32_t>((size_t)chunk); nlen = c.take<int32_t>(2 * (size_t)chunk);
            sbuf = c.take<uint8_t>((size_t)chunk); viol = c.take<unsigned>(1);
        })) return -1;
    std::vector<int32_t> h_nlen(2 * (size_t)chunk);
    unsigned h_viol = 0;
    pmx_config_t cfg1 = *cfg;
    cfg1.want &= ~(PMX_WANT_STATS | PMX_WANT_CIGAR);            // (the score pass)
    const double bound = frameshift_trace_bound();
    g_fswin_parts = 0;
    HIP_OR_RET(hipMemsetAsync(viol, 0, sizeof(unsigned), st));
    auto violated = [&]() -> int {
        if (!h_viol) return 0;
        set_err("window proof violated: %u records of the narrowed trace pass differ from the score pass", h_viol);
        return -1;
    };
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cn = std::min<int64_t>(chunk, n - c0);
        SlotPlan p1 = fr;
        if (p1.d_byte) p1.d_byte += c0;
        uint8_t *won = d_strand_out ? d_strand_out + c0 : sbuf;
        int rc = pairs_run_folded(&cfg1, Q, R, cn, d_pairs + c0, p1, max_qlen, max_rlen, rec1, nullptr, won, st, cn);
        if (rc) return rc;
        rc = pmx_launch_fsref_window(d_pairs + c0, rec1, won, cn, Q->d_buf, Q->d_off, Q->count, Q->bytes, R->d_off, R->count, R->bytes,
                                     dm.d, cfg->open, cfg->extend, fr.frameshift, npairs, ashift, nlen, st);
        if (rc) { set_err("frameshift window kernel launch failed (%d)", rc); return rc < 0 ? rc : -1; }
        HIP_OR_RET(hipMemcpyAsync(h_nlen.data(), nlen, sizeof(int32_t) * 2 * (size_t)cn, hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipMemcpyAsync(&h_viol, viol, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipStreamSynchronize(st));
        if (violated()) return -1;
        for (int64_t k = 0; k < cn; ++k) {
            const int32_t nq = std::max<int32_t>(1, h_nlen[2 * k]), nr = std::max<int32_t>(1, h_nlen[2 * k + 1]);
            const size_t tps = frameshift_trace_bytes_per_slot(true, nq, nr);
            if (4.0 * (double)tps > bound) { (void)frameshift_trace_bound_check(tps, nq, nr); return -1; }      // (the existing text, the narrowed figures)
        }
        SlotPlan p2 = fr;
        p2.first = 0; p2.per = 1;
        for (int64_t p0 = 0; p0 < cn;) {
            int32_t mq = 1, mr = 1; int64_t pn = 0;
            while (p0 + pn < cn) {
                const int32_t nq = std::max(mq, h_nlen[2 * (p0 + pn)]), nr = std::max(mr, h_nlen[2 * (p0 + pn) + 1]);
                if (pn > 0 && (double)((pn + 4) / 4 * 4) * (double)frameshift_trace_bytes_per_slot(true, nq, nr) > bound) break;
                mq = nq; mr = nr; ++pn;
            }
            const int64_t g0 = c0 + p0;
            p2.d_byte = won + p0;
            rc = pairs_run_codons_cigar(cfg, Q, R, pn, npairs + p0, mq, mr, d_out + g0, nullptr, d_stats ? d_stats + g0 : nullptr,
                                        d_beg ? d_beg + 2 * g0 : nullptr, d_text, capacity, d_text_off + g0, st, pn, p2, g0 > 0);
            if (rc) return rc;
            p0 += pn; ++g_fswin_parts;
        }
        rc = pmx_launch_fsref_rebase(rec1, ashift, cn, d_out + c0, d_beg ? d_beg + 2 * c0 : nullptr, viol, st);
        if (rc) { set_err("frameshift rebase kernel launch failed (%d)", rc); return rc; }
    }
    HIP_OR_RET(hipMemcpyAsync(&h_viol, viol, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    return violated();
}

extern "C" int pmx_align_pairs_frameshift_ref_cigar_long_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                                int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int strand_mode,
                                                                int32_t frameshift, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                                pmx_record_t *d_out, uint8_t *d_strand_out, pmx_stats_t *d_stats, int32_t *d_beg,
                                                                char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off,
                                                                void *stream, const pmx_pairs_opts_t *opts)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts) || frameshift_check(cfg, strand_mode, d_strand, frameshift, code, &fr, true, true) ||
        frameshift_cigar_outputs_check(cfg, d_stats, d_cigar_text, cigar_capacity, d_cigar_off) || byte_out_check(fr, n > 0, d_strand_out)) return -1;
    if (n == 0) return 0;
    if (frameshift_rows_check(max_qlen, true) || pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats != nullptr, true)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_codons_cigar_windowed(cfg, Q, R, n, d_pairs, max_qlen, max_rlen, d_out, d_strand_out, d_stats, d_beg, d_cigar_text, cigar_capacity,
                                           d_cigar_off, (hipStream_t)stream, pairs_chunk(n, max_qlen, max_rlen, opts, fr.per), fr);
}

extern "C" int pmx_gather_pairs_codons_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                              const uint8_t *d_strand, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                              uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                              uint8_t *d_ok, void *stream)
{
    return gather_pairs_hook(Q, R, n, d_pairs, SlotPlan::CODONS, false, d_strand, code, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream);
}

extern "C" int pmx_gather_pairs_codons_ref_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                                  const uint8_t *d_strand, const uint8_t *code, int32_t max_qlen, int32_t max_rlen,
                                                  uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                                  uint8_t *d_ok, void *stream)
{
    return gather_pairs_hook(Q, R, n, d_pairs, SlotPlan::CODONS, true, d_strand, code, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream);
}

// ---- strands and CIGAR output (pmx_align_pairs_ex[_device], pmx_gather_pairs_device) ----
extern "C" void pmx_complement_table(uint8_t table[256]) { if (table) pmx_complement_table_host(table); }

// What the _ex entries refuse about their outputs, before any GPU work.  text: d_cigar_text / cigar_buf.
static int pairs_ex_outputs_check(const pmx_config_t *cfg, const void *beg, const void *text, int64_t capacity, const void *text_off)
{
    if (cfg->want & PMX_WANT_CIGAR) {
        if (cfg->want & PMX_WANT_STATS) { set_err("PMX_WANT_CIGAR together with PMX_WANT_STATS is not offered by set batches (the walk does one of the two)"); return -1; }
        if (!text || !text_off) { set_err("null cigar output"); return -1; }
        if (capacity < 0) { set_err("negative cigar_capacity"); return -1; }
    } else if (beg || text || text_off) { set_err("begins and CIGAR buffers need PMX_WANT_CIGAR in cfg->want"); return -1; }
    return 0;
}

// The CIGAR road of a set batch: every chunk's packed windows through cigar_device_run, which fixes the chunk's bad pairs up and
// continues the text behind the chunks before it (d_cigar_off[c0], left by the previous chunk on the same stream).  The caller has
// checked the road's window.
static int pairs_run_cigar(const pmx_config_t *cfg, const DevMat &dm, const pmx_seqset *Q, const pmx_seqset *R, int64_t n,
                           const pmx_pair_t *d_pairs, const uint8_t *d_strand, int32_t max_qlen, int32_t max_rlen,
                           pmx_record_t *d_out, int32_t *d_beg, char *d_text, int64_t capacity, int64_t *d_text_off, hipStream_t st, int64_t chunk)
{
    return pairs_run(Q, R, n, d_pairs, 0, PMX_PAIRS_LIST, SlotPlan(d_strand), max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            CigarChunkOf set; set.ok = b.ok; set.beg = d_beg ? d_beg + 2 * c0 : nullptr; set.continues = c0 > 0;
            const int rc = cigar_device_run(cfg, dm, cn, b.q, b.qoff, b.r, b.roff, max_qlen, max_rlen, 0, d_out + c0,
                                            d_text, capacity, d_text_off + c0, st, set);
            if (rc == 1) set_err_no_cigar_road();
            return rc == 1 ? -1 : rc;
        });
}

// Both roads behind the checks the two _ex entries share; asynchronous on `st`.
static int pairs_ex_run(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs,
                        const uint8_t *d_strand, int32_t max_qlen, int32_t max_rlen, pmx_record_t *d_out, pmx_stats_t *d_stats_out,
                        int32_t *d_beg, char *d_text, int64_t capacity, int64_t *d_text_off, hipStream_t st, const pmx_pairs_opts_t *opts)
{
    const int64_t chunk = pairs_chunk(n, max_qlen, max_rlen, opts);
    if (!(cfg->want & PMX_WANT_CIGAR))
        return pairs_run_scores(cfg, Q, R, n, d_pairs, 0, SlotPlan(d_strand), max_qlen, max_rlen, d_out, d_stats_out, st, chunk);
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    if (!cigar_device_eligible(cfg, dm, chunk, max_qlen, max_rlen)) { set_err_no_cigar_road(); return -1; }
    return pairs_run_cigar(cfg, dm, Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_out, d_beg, d_text, capacity, d_text_off, st, chunk);
}

extern "C" int pmx_align_pairs_ex_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                         int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_strand, int32_t max_qlen, int32_t max_rlen,
                                         pmx_record_t *d_out, pmx_stats_t *d_stats_out, int32_t *d_beg,
                                         char *d_cigar_text, int64_t cigar_capacity, int64_t *d_cigar_off, void *stream, const pmx_pairs_opts_t *opts)
{
    if (listed_entry_check(cfg, Q, R, n, d_pairs, d_out, opts) || pairs_ex_outputs_check(cfg, d_beg, d_cigar_text, cigar_capacity, d_cigar_off)) return -1;
    if (n == 0) return 0;
    if (pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_stats_out != nullptr, true)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_ex_run(cfg, Q, R, n, d_pairs, d_strand, max_qlen, max_rlen, d_out, d_stats_out, d_beg, d_cigar_text, cigar_capacity, d_cigar_off,
                        (hipStream_t)stream, opts);
}

extern "C" int pmx_gather_pairs_device(const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs,
                                       const uint8_t *d_strand, int32_t max_qlen, int32_t max_rlen,
                                       uint8_t *d_qout, int64_t q_capacity, int64_t *d_qoff, uint8_t *d_rout, int64_t r_capacity, int64_t *d_roff,
                                       uint8_t *d_ok, void *stream)
{
    return gather_pairs_hook(Q, R, n, d_pairs, SlotPlan::BYTES, false, d_strand, nullptr, max_qlen, max_rlen, d_qout, q_capacity, d_qoff, d_rout, r_capacity, d_roff, d_ok, stream);
}

// The all-pairs window [first, first + count) of a set: 0, or -1 with the cause.
static int all_pairs_window(int64_t nseq, int64_t first, int64_t count)
{
    if (first < 0 || count < 0) { set_err("negative first or count"); return -1; }
    const int64_t total = pmx_all_pairs_count(nseq);
    if (total < 0) return -1;
    if (first > total || count > total - first) {
        set_err("pairs %lld .. %lld are beyond the %lld pairs of %lld sequences", (long long)first, (long long)first + (long long)count - 1, (long long)total, (long long)nseq);
        return -1;
    }
    return 0;
}

extern "C" int pmx_align_all_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *S, int64_t first, int64_t count,
                                          int32_t max_len, pmx_record_t *d_out, pmx_stats_t *d_stats_out, void *stream,
                                          const pmx_pairs_opts_t *opts)
{
    if (!S) { set_err("null sequence set"); return -1; }
    if (all_pairs_window(S->count, first, count)) return -1;
    if (count > 0 && !d_out) { set_err("null records"); return -1; }
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg)) return -1;
    if (count == 0) return 0;
    if (pairs_check(cfg, S, S, opts, max_len, max_len, d_stats_out != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return pairs_run_scores(cfg, S, S, count, nullptr, first, SlotPlan(), max_len, max_len, d_out, d_stats_out, (hipStream_t)stream, pairs_chunk(count, max_len, max_len, opts));
}

extern "C" int pmx_all_pairs_enumerate_device(int64_t nseq, int64_t first, int64_t count, pmx_pair_t *d_pairs, void *stream)
{
    if (all_pairs_window(nseq, first, count)) return -1;
    if (count == 0) return 0;
    if (!d_pairs) { set_err("null pairs"); return -1; }
    const int rc = pmx_launch_all_pairs_enumerate(nseq, first, count, d_pairs, (hipStream_t)stream);
    if (rc) { set_err("pair enumeration launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
    return 0;
}

// One side of a descriptor against host offsets: nullptr, or what is wrong with it; *len = the resolved length.
static const char *host_resolve_side(const std::vector<int64_t> &off, int64_t count, int64_t idx, int32_t beg, int32_t len, int64_t *out)
{
    if (idx < 0 || idx >= count) return "index outside the set";
    if (beg < 0) return "negative window start";
    if (len < -1) return "negative window length";
    const int64_t slen = off[idx + 1] - off[idx], l = len < 0 ? slen - beg : (int64_t)len;
    if (l < 1) return "empty window";
    if ((int64_t)beg + l > slen) return "window reaches past the end of the sequence";
    if (l > INT32_MAX) return "window longer than 2^31 - 1";
    *out = l;
    return nullptr;
}

// Pairs [a, e) against the host offsets: the first bad one (what is wrong with which side), or the extreme window lengths.
struct PairScan { int64_t bad = -1; const char *what = nullptr, *side = nullptr; int64_t mq = 1, mr = 1, mnr = INT32_MAX, symbols = 0; };
static PairScan scan_pairs(const pmx_seqset *Q, const pmx_seqset *R, const pmx_pair_t *pairs, int64_t a, int64_t e)
{
    PairScan s;
    for (int64_t k = a; k < e; ++k) {
        int64_t ql = 0, rl = 0;
        const char *what = host_resolve_side(Q->h_off, Q->count, pairs[k].q, pairs[k].q_beg, pairs[k].q_len, &ql);
        const char *side = "query";
        if (!what) { what = host_resolve_side(R->h_off, R->count, pairs[k].r, pairs[k].r_beg, pairs[k].r_len, &rl); side = "reference"; }
        if (what) { s.bad = k; s.what = what; s.side = side; return s; }
        s.mq = ql > s.mq ? ql : s.mq; s.mr = rl > s.mr ? rl : s.mr; s.mnr = rl < s.mnr ? rl : s.mnr; s.symbols += ql + rl;
    }
    return s;
}

// The longest good windows of a batch over a set without host offsets (one small kernel and one synchronisation).
static int device_maxlens(const pmx_seqset *Q, const pmx_seqset *R, const pmx_pair_t *d_pairs, int64_t n, int32_t *mq, int32_t *mr, hipStream_t st)
{
    int32_t *d = nullptr, h[2] = {0, 0};
    if (scratch_reserve(256, (void **)&d, SCR_PGEN)) return -1;
    HIP_OR_RET(hipMemsetAsync(d, 0, 2 * sizeof(int32_t), st));
    const int rc = pmx_launch_pairs_maxlen(d_pairs, n, Q->d_off, Q->count, Q->bytes, R->d_off, R->count, R->bytes, d, st);
    if (rc) { set_err("length scan launch failed (%d)", rc); return rc; }
    HIP_OR_RET(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    *mq = h[0] > 0 ? h[0] : 1; *mr = h[1] > 0 ? h[1] : 1;        // (no good window at all: every record will be flagged)
    return 0;
}

// The lengths an enumerated window -- pairs [first, first + n) of shape PMX_PAIRS_TRIANGLE (R == Q) / PMX_PAIRS_RECT, whole sequences --
// is run with, both ways the enumerating host entries (pmx_align_all_pairs, pmx_search_pairs, pmx_search_topk) find them.
// Sets with host offsets: the longest query and reference (at most 2^31 - 1) and the shortest reference (at least 1) of the whole sets.
// When some sequence cannot be a whole-sequence window, the window is walked row by row for the first pair that touches one -- the query
// before the reference, the row's first such column -- and that pair, numbered from `first`, is the call's failure.
struct SetLens { int32_t mq = 1, mr = 1, mnr = INT32_MAX; };           // (as created: wrapped sets before the device pass; with_sort_hint sees nothing to sort by)
static int window_host_lens(const pmx_seqset *Q, const pmx_seqset *R, int shape, int64_t first, int64_t n, SetLens *m)
{
    std::vector<int64_t> oddq, oddr; int64_t mq = 1, mnq = INT32_MAX, mr = 1, mnr = INT32_MAX;
    // a set's extreme lengths; odd: the sequences that cannot be whole-sequence windows (empty, or beyond 2^31 - 1), ascending
    auto lengths = [](const pmx_seqset *S, int64_t *mx, int64_t *mn, std::vector<int64_t> *odd) {
        for (int64_t k = 0; k < S->count; ++k) {
            const int64_t l = S->h_off[k + 1] - S->h_off[k];
            if (l < 1 || l > INT32_MAX) odd->push_back(k);
            *mx = l > *mx ? l : *mx; *mn = l < *mn ? l : *mn;
        }
    };
    try {
        lengths(Q, &mq, &mnq, &oddq);
        if (R != Q) lengths(R, &mr, &mnr, &oddr); else { mr = mq; mnr = mnq; oddr = oddq; }
    } catch (const std::bad_alloc &) { set_err("out of memory"); return -1; }
    m->mq = (int32_t)std::min<int64_t>(mq, INT32_MAX); m->mr = (int32_t)std::min<int64_t>(mr, INT32_MAX); m->mnr = (int32_t)std::max<int64_t>(mnr, 1);
    if (oddq.empty() && oddr.empty()) return 0;
    const bool tri = shape == PMX_PAIRS_TRIANGLE;
    int64_t i = tri ? 0 : first / R->count, j = tri ? 0 : first - i * R->count, l = 0;
    if (tri) (void)pmx_all_pairs_index(Q->count, first, &i, &j);
    for (int64_t p = first, end = first + n; p < end; ++i, j = tri ? i + 1 : 0) {
        const int64_t jb = std::min<int64_t>(R->count, j + (end - p));      // columns [j, jb) of row i are pairs [p, p + jb - j)
        const char *what = host_resolve_side(Q->h_off, Q->count, i, 0, -1, &l);
        const char *side = "query";
        int64_t jbad = j;
        if (!what) {
            const auto it = std::lower_bound(oddr.begin(), oddr.end(), j);
            if (it != oddr.end() && *it < jb) { jbad = *it; what = host_resolve_side(R->h_off, R->count, jbad, 0, -1, &l); side = "reference"; }
        }
        if (what) { set_err("pair %lld (%lld, %lld): %s: %s", (long long)(p + (jbad - j) - first), (long long)i, (long long)jbad, side, what); return -1; }
        p += jb - j;
    }
    return 0;
}
// Wrapped sets: the longest sequence of either set, found on the device, and what a PSSM refuses about it.
static int window_device_lens(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, SetLens *m, hipStream_t st)
{
    int32_t unused = 0;
    if (device_maxlens(Q, Q, nullptr, Q->count, &m->mq, &unused, st)) return -1;
    m->mr = m->mq;
    if (R != Q && device_maxlens(R, R, nullptr, R->count, &m->mr, &unused, st)) return -1;
    return pssm_batch_check(cfg->matrix, m->mq, m->mq);
}

// Device records (and statistics) back to the host; a flagged record -- a set without host offsets was validated on the device -- is
// the call's failure.
static int pairs_copy_back(int64_t n, const pmx_record_t *drec, const pmx_stats_t *dst, pmx_record_t *out, pmx_stats_t *stats_out, bool scan_flags, hipStream_t st)
{
    HIP_OR_RET(hipMemcpyAsync(out, drec, sizeof(pmx_record_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (dst) HIP_OR_RET(hipMemcpyAsync(stats_out, dst, sizeof(pmx_stats_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    if (scan_flags)
        for (int64_t k = 0; k < n; ++k)
            if (out[k].flags & PMX_FLAG_BAD_PAIR) { set_err("pair %lld: bad descriptor (index, window or length)", (long long)k); return -1; }
    return 0;
}

// Listed pairs over a set with host offsets, the descriptors below `end` good: the first whose query window has fewer than three
// nucleotides -- no codon stream --, refused with its number; 0 when there is none.  ref (the _frameshift_ref entries): S is the
// reference set and the window the reference's.
static int short_window_check(const pmx_seqset *S, const pmx_pair_t *pairs, int64_t end, bool ref = false)
{
    for (int64_t k = 0; k < end; ++k) {
        const pmx_pair_t &p = pairs[k];
        const int64_t idx = ref ? p.r : p.q, beg = ref ? p.r_beg : p.q_beg, len = ref ? p.r_len : p.q_len;
        const int64_t W = len < 0 ? S->h_off[(size_t)idx + 1] - S->h_off[(size_t)idx] - beg : len;
        if (W < 3) { set_err("pair %lld: %s: a window of %lld nucleotides has no codon", (long long)k, ref ? "reference" : "query", (long long)W); return -1; }
    }
    return 0;
}

// The one host road over listed pairs, behind the entries' own argument checks: the validation of the bytes per pair (strands; FRAMES:
// frames), the descriptors against host offsets -- the scan cut into slices on helper threads for large batches, merged in pair order, so
// the lowest bad pair is the one named --, the maxima in letters, the upload of 32 (+ 1) bytes per pair, the maxima of wrapped sets from
// the device -- then run(cfg, d_pairs, max_qlen, max_rlen, d_rec, d_stats, d_byte_out, st), then the winners' bytes (byte_out, may be
// NULL) and the records back.  plan.d_byte: the uploaded bytes, where there are any.  scan_flags: the records' flags are scanned for
// bad pairs even with host offsets -- a pair without a frame or a codon is found on the device only.  lens_check(max_qlen, max_rlen,
// known): what the entry refuses about the maxima, asked before any GPU work (known: the sets have host offsets) and again for wrapped
// sets.  hint: the run's configuration carries the sort hint of the host lengths.  *symbols (may be NULL): the letters of all windows,
// for wrapped sets n times the maxima -- what a text estimate starts from.
template <typename LensCheck, typename Run>
static int listed_pairs_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *pairs,
                             const uint8_t *byte_in, SlotPlan &plan, pmx_record_t *out, pmx_stats_t *stats_out, uint8_t *byte_out,
                             const pmx_pairs_opts_t *opts, bool ex, bool hint, bool scan_flags, int64_t *symbols, LensCheck lens_check, Run run)
{
    const bool codons = plan.kind == SlotPlan::CODONS, frames = plan.kind == SlotPlan::FRAMES;
    if (byte_in)
        for (int64_t k = 0; k < n; ++k)
            if (byte_in[k] > (frames ? 5 : 1)) {
                set_err(frames ? "pair %lld: frame byte %d is outside 0 .. 5" : "pair %lld: strand byte %d is neither 0 nor 1", (long long)k, (int)byte_in[k]);
                return -1;
            }
    const bool host_offsets = !Q->h_off.empty() && !R->h_off.empty();
    int32_t q32 = 1, r32 = 1, mnr = INT32_MAX;
    if (host_offsets) {
        // large batches: the scan is a few nanoseconds per pair of random reads into the offsets -- measured at 2.1 ms per million
        // pairs on one core, of a 6.9 ms call -- so it is cut into slices on helper threads, merged in pair order
        const int T = n >= 262144 ? 4 : 1;
        PairScan part[4], s;
        std::future<void> helper[4];
        for (int t = 1; t < T; ++t) {
            const int64_t a = n * t / T, e = n * (t + 1) / T;
            try { helper[t] = std::async(std::launch::async, [&, t, a, e]() { part[t] = scan_pairs(Q, R, pairs, a, e); }); }
            catch (const std::system_error &) { part[t] = scan_pairs(Q, R, pairs, a, e); }          // no helper thread to be had: scan inline
        }
        part[0] = scan_pairs(Q, R, pairs, 0, n / T);
        for (int t = 1; t < T; ++t) if (helper[t].valid()) helper[t].get();
        for (int t = 0; t < T && s.bad < 0; ++t) {
            s.bad = part[t].bad; s.side = part[t].side; s.what = part[t].what;
            s.mq = std::max(s.mq, part[t].mq); s.mr = std::max(s.mr, part[t].mr); s.mnr = std::min(s.mnr, part[t].mnr); s.symbols += part[t].symbols;
        }
        if (codons && short_window_check(plan.ref ? R : Q, pairs, s.bad >= 0 ? s.bad : n, plan.ref)) return -1;
        if (s.bad >= 0) { set_err("pair %lld: %s: %s", (long long)s.bad, s.side, s.what); return -1; }
        q32 = (int32_t)s.mq; r32 = (int32_t)s.mr; mnr = (int32_t)s.mnr;
        if (symbols) *symbols = s.symbols;
        plan.to_letters(&q32, &r32, &mnr);
    }
    if (lens_check(q32, r32, host_offsets) || pairs_check(cfg, Q, R, opts, q32, r32, stats_out != nullptr, ex)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    pmx_pair_t *dp = nullptr; pmx_record_t *drec = nullptr; pmx_stats_t *dst = nullptr;
    const size_t up_bytes = (sizeof(pmx_pair_t) * (size_t)n + 255) & ~(size_t)255;          // descriptors, then the bytes in, then out
    if (scratch_reserve(up_bytes + 2 * (size_t)n, (void **)&dp, SCR_PUP) || scratch_reserve(sizeof(pmx_record_t) * (size_t)n, (void **)&drec, SCR_PREC) ||
        (stats && scratch_reserve(sizeof(pmx_stats_t) * (size_t)n, (void **)&dst, SCR_PST))) return -1;
    uint8_t *dbin = (uint8_t *)dp + up_bytes, *dbout = dbin + n;
    HIP_OR_RET(hipMemcpyAsync(dp, pairs, sizeof(pmx_pair_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (byte_in) { HIP_OR_RET(hipMemcpyAsync(dbin, byte_in, (size_t)n, hipMemcpyHostToDevice, st)); plan.d_byte = dbin; }
    pmx_config_t cfg_s = *cfg;
    if (host_offsets) { if (hint) cfg_s = with_sort_hint(cfg, mnr, r32, n); }
    else {
        if (device_maxlens(Q, R, dp, n, &q32, &r32, st)) return -1;
        if (symbols) *symbols = (int64_t)n * ((int64_t)q32 + r32);           // (wrapped sets: the lengths stayed on the device)
        plan.to_letters(&q32, &r32);
        if (lens_check(q32, r32, true) || pssm_batch_check(cfg->matrix, q32, q32)) return -1;
    }
    const int rc = run(&cfg_s, dp, q32, r32, drec, dst, dbout, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    if (byte_out) HIP_OR_RET(hipMemcpyAsync(byte_out, dbout, (size_t)n, hipMemcpyDeviceToHost, st));
    return pairs_copy_back(n, drec, dst, out, stats_out, scan_flags || !host_offsets, st);
}

// The host entries over listed pairs.  ex: pmx_align_pairs_ex -- strand bytes (may be NULL), and with PMX_WANT_CIGAR the begins (may be
// NULL) and the text, a HostText stage of half a byte per symbol + 16 per pair.
// both: pmx_align_pairs_both -- PMX_STRAND_BOTH, the winners' strand bytes into strand_out.
static int pairs_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *pairs, const uint8_t *strand,
                      pmx_record_t *out, pmx_stats_t *stats_out, int32_t *beg, char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts, bool ex,
                      bool both = false, uint8_t *strand_out = nullptr)
{
    SlotPlan plan;                                        // both: the two strands; else PLAIN, and d_byte the strand bytes once they are on the device
    if (both) plan.strands(PMX_STRAND_BOTH);
    if (listed_entry_check(cfg, Q, R, n, pairs, out, opts, both ? &plan : nullptr, strand_out)) return -1;
    if (both && (pairs_both_want_check(cfg) || strand_mode_check(cfg, PMX_STRAND_BOTH, &plan))) return -1;
    if (ex && pairs_ex_outputs_check(cfg, beg, cigar_buf, 0, cigar_off)) return -1;
    const bool cigar = ex && (cfg->want & PMX_WANT_CIGAR) != 0;
    if (cigar) { *cigar_buf = nullptr; cigar_off[0] = 0; }
    if (n == 0) return 0;
    int64_t symbols = 0;
    HostText text; DevBuf<int32_t> dbeg;
    const int rc = listed_pairs_host(cfg, Q, R, n, pairs, strand, plan, out, stats_out, strand_out, opts, ex, true, false, &symbols,
        [](int32_t, int32_t, bool) { return 0; },
        [&](const pmx_config_t *c, const pmx_pair_t *dp, int32_t q32, int32_t r32, pmx_record_t *drec, pmx_stats_t *dst, uint8_t *dsout, hipStream_t st) -> int {
            if (both) return pairs_run_folded(c, Q, R, n, dp, plan, q32, r32, drec, dst, dsout, st, pairs_chunk(n, q32, r32, opts, plan.per));
            if (!cigar) return pairs_ex_run(c, Q, R, n, dp, plan.d_byte, q32, r32, drec, dst, nullptr, nullptr, 0, nullptr, st, opts);
            if (beg && dbeg.try_alloc(2 * (size_t)n)) { set_err("out of device memory"); return -2; }
            if (text.alloc(n, symbols / 2 + 16 * n + 256)) return -2;
            return text.run(n, cigar_off, &st, [&](char *d_text, int64_t capacity, int64_t *d_text_off) {
                return pairs_ex_run(c, Q, R, n, dp, plan.d_byte, q32, r32, drec, nullptr, dbeg.p, d_text, capacity, d_text_off, st, opts);
            });
        });
    if (rc || !cigar) return rc;
    if (beg) HIP_OR_RET(hipMemcpy(beg, dbeg.p, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    return text.to_block(cigar_off[n], cigar_buf);
}

extern "C" int pmx_align_pairs(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                               int64_t n, const pmx_pair_t *pairs, pmx_record_t *out, pmx_stats_t *stats_out, const pmx_pairs_opts_t *opts)
{
    return pairs_host(cfg, Q, R, n, pairs, nullptr, out, stats_out, nullptr, nullptr, nullptr, opts, false);
}

extern "C" int pmx_align_pairs_ex(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                  int64_t n, const pmx_pair_t *pairs, const uint8_t *strand,
                                  pmx_record_t *out, pmx_stats_t *stats_out, int32_t *beg,
                                  char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts)
{
    return pairs_host(cfg, Q, R, n, pairs, strand, out, stats_out, beg, cigar_buf, cigar_off, opts, true);
}

extern "C" int pmx_align_pairs_both(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                    int64_t n, const pmx_pair_t *pairs, pmx_record_t *out, pmx_stats_t *stats_out, uint8_t *strand_out,
                                    const pmx_pairs_opts_t *opts)
{
    return pairs_host(cfg, Q, R, n, pairs, nullptr, out, stats_out, nullptr, nullptr, nullptr, opts, false, true, strand_out);
}



// The host entries over listed pairs with a translated side (ref false: pmx_align_pairs_translated, true: pmx_align_pairs_translated_ref).
static int align_pairs_frames_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                   int64_t n, const pmx_pair_t *pairs, const uint8_t *frame, int frame_mode, const uint8_t *code,
                                   pmx_record_t *out, pmx_stats_t *stats_out, uint8_t *frame_out, const pmx_pairs_opts_t *opts, bool ref)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, pairs, out, opts) || frames_check(cfg, frame_mode, frame, code, &fr, ref) ||
        byte_out_check(fr, n > 0, frame_out)) return -1;
    if (n == 0) return 0;
    return listed_pairs_host(cfg, Q, R, n, pairs, frame, fr, out, stats_out, frame_out, opts, false, true, true, nullptr,
        [](int32_t, int32_t, bool) { return 0; },
        [&](const pmx_config_t *c, const pmx_pair_t *dp, int32_t q32, int32_t r32, pmx_record_t *drec, pmx_stats_t *dst, uint8_t *dfout, hipStream_t st) {
            return pairs_run_folded(c, Q, R, n, dp, fr, q32, r32, drec, dst, dfout, st, pairs_chunk(n, q32, r32, opts, fr.per));
        });
}

extern "C" int pmx_align_pairs_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                          int64_t n, const pmx_pair_t *pairs, const uint8_t *frame, int frame_mode, const uint8_t *code,
                                          pmx_record_t *out, pmx_stats_t *stats_out, uint8_t *frame_out, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frames_host(cfg, Q, R, n, pairs, frame, frame_mode, code, out, stats_out, frame_out, opts, false);
}

extern "C" int pmx_align_pairs_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                              int64_t n, const pmx_pair_t *pairs, const uint8_t *frame, int frame_mode, const uint8_t *code,
                                              pmx_record_t *out, pmx_stats_t *stats_out, uint8_t *frame_out, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frames_host(cfg, Q, R, n, pairs, frame, frame_mode, code, out, stats_out, frame_out, opts, true);
}

// The host entries over listed pairs of the frameshift-aware alignment.  traceback (pmx_align_pairs_frameshift_cigar): the
// traceback road in place of the score road, and a HostText stage of 32 bytes per pair.
static int align_pairs_frameshift_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                       int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                       int32_t frameshift, const uint8_t *code, pmx_record_t *out, uint8_t *strand_out,
                                       const pmx_pairs_opts_t *opts, bool traceback,
                                       pmx_stats_t *stats_out, int32_t *beg, char **cigar_buf, int64_t *cigar_off,
                                       bool ref = false /* pmx_align_pairs_frameshift_ref[_cigar]: the stream is the reference's */,
                                       bool windowed = false /* pmx_align_pairs_frameshift_ref_cigar_long: the windowed road, no bound on the un-narrowed shape */)
{
    SlotPlan fr;
    if (listed_entry_check(cfg, Q, R, n, pairs, out, opts) || frameshift_check(cfg, strand_mode, strand, frameshift, code, &fr, traceback, ref) ||
        (traceback && frameshift_cigar_outputs_check(cfg, stats_out, cigar_buf, 0, cigar_off)) || byte_out_check(fr, n > 0, strand_out)) return -1;
    if (traceback) { *cigar_buf = nullptr; cigar_off[0] = 0; }
    if (n == 0) return 0;
    HostText text; DevBuf<int32_t> dbeg;
    const int rc = listed_pairs_host(cfg, Q, R, n, pairs, strand, fr, out, stats_out, strand_out, opts, traceback, false, true, nullptr,
        [&](int32_t mq, int32_t mr, bool known) {
            return frameshift_rows_check(mq, ref) || (traceback && !windowed && known && frameshift_trace_bound_check(frameshift_trace_bytes_per_slot(ref, mq, mr), mq, mr)) ? -1 : 0;
        },
        [&](const pmx_config_t *c, const pmx_pair_t *dp, int32_t q32, int32_t r32, pmx_record_t *drec, pmx_stats_t *dst, uint8_t *dsout, hipStream_t st) -> int {
            const int64_t chunk = pairs_chunk(n, q32, r32, opts, fr.per);
            if (!traceback) return pairs_run_folded(c, Q, R, n, dp, fr, q32, r32, drec, nullptr, dsout, st, chunk);
            if (beg && dbeg.try_alloc(2 * (size_t)n)) { set_err("out of device memory"); return -2; }
            if (text.alloc(n, 32 * n + 256)) return -2;             // (the run-length text of a hit is a few runs; a batch of noise runs twice)
            return text.run(n, cigar_off, &st, [&](char *d_text, int64_t capacity, int64_t *d_text_off) {
                return windowed ? pairs_run_codons_cigar_windowed(c, Q, R, n, dp, q32, r32, drec, dsout, dst, dbeg.p, d_text, capacity, d_text_off, st, chunk, fr)
                                : pairs_run_codons_cigar(c, Q, R, n, dp, q32, r32, drec, dsout, dst, dbeg.p, d_text, capacity, d_text_off, st, chunk, fr);
            });
        });
    if (rc || !traceback) return rc;
    if (beg) HIP_OR_RET(hipMemcpy(beg, dbeg.p, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    return text.to_block(cigar_off[n], cigar_buf);
}

extern "C" int pmx_align_pairs_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                          int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                          int32_t frameshift, const uint8_t *code,
                                          pmx_record_t *out, uint8_t *strand_out, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frameshift_host(cfg, Q, R, n, pairs, strand, strand_mode, frameshift, code, out, strand_out, opts, false,
                                       nullptr, nullptr, nullptr, nullptr);
}

extern "C" int pmx_align_pairs_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                              int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                              int32_t frameshift, const uint8_t *code,
                                              pmx_record_t *out, uint8_t *strand_out, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frameshift_host(cfg, Q, R, n, pairs, strand, strand_mode, frameshift, code, out, strand_out, opts, false,
                                       nullptr, nullptr, nullptr, nullptr, true);
}

extern "C" int pmx_align_pairs_frameshift_cigar(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                                int32_t frameshift, const uint8_t *code,
                                                pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out, int32_t *beg,
                                                char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frameshift_host(cfg, Q, R, n, pairs, strand, strand_mode, frameshift, code, out, strand_out, opts, true,
                                       stats_out, beg, cigar_buf, cigar_off);
}

extern "C" int pmx_align_pairs_frameshift_ref_cigar(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                    int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                                    int32_t frameshift, const uint8_t *code,
                                                    pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out, int32_t *beg,
                                                    char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frameshift_host(cfg, Q, R, n, pairs, strand, strand_mode, frameshift, code, out, strand_out, opts, true,
                                       stats_out, beg, cigar_buf, cigar_off, true);
}

extern "C" int pmx_align_pairs_frameshift_ref_cigar_long(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R,
                                                         int64_t n, const pmx_pair_t *pairs, const uint8_t *strand, int strand_mode,
                                                         int32_t frameshift, const uint8_t *code,
                                                         pmx_record_t *out, uint8_t *strand_out, pmx_stats_t *stats_out, int32_t *beg,
                                                         char **cigar_buf, int64_t *cigar_off, const pmx_pairs_opts_t *opts)
{
    return align_pairs_frameshift_host(cfg, Q, R, n, pairs, strand, strand_mode, frameshift, code, out, strand_out, opts, true,
                                       stats_out, beg, cigar_buf, cigar_off, true, true);
}

extern "C" int pmx_align_all_pairs(const pmx_config_t *cfg, const pmx_seqset_t *S, int64_t first, int64_t count,
                                   pmx_record_t *out, pmx_stats_t *stats_out, const pmx_pairs_opts_t *opts)
{
    if (!S) { set_err("null sequence set"); return -1; }
    if (all_pairs_window(S->count, first, count)) return -1;
    if (count > 0 && !out) { set_err("null records"); return -1; }
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg)) return -1;
    if (count == 0) return 0;
    const bool host_offsets = !S->h_off.empty();
    SetLens m;
    if (host_offsets && window_host_lens(S, S, PMX_PAIRS_TRIANGLE, first, count, &m)) return -1;
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    if (pairs_check(cfg, S, S, opts, m.mq, m.mq, stats_out != nullptr)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    pmx_record_t *drec = nullptr; pmx_stats_t *dst = nullptr;
    if (scratch_reserve(sizeof(pmx_record_t) * (size_t)count, (void **)&drec, SCR_PREC) ||
        (stats && scratch_reserve(sizeof(pmx_stats_t) * (size_t)count, (void **)&dst, SCR_PST))) return -1;
    const pmx_config_t cfg_s = with_sort_hint(cfg, m.mnr, m.mq, count);      // (wrapped sets: no host lengths yet, and no hint from them)
    if (!host_offsets && window_device_lens(cfg, S, S, &m, st)) return -1;
    const int rc = pairs_run_scores(&cfg_s, S, S, count, nullptr, first, SlotPlan(), m.mq, m.mq, drec, dst, st, pairs_chunk(count, m.mq, m.mq, opts));
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    return pairs_copy_back(count, drec, dst, out, stats_out, !host_offsets, st);
}

// ==================================================================== set search ===
// pmx_search_pairs[_device] (semantics: include/parasail_amd.h): the chunk loop of the set batches with a body that keeps
// the chunk's records in scratch, asks pmx_launch_select for the positions of those at or above min_score and appends them -- descriptor,
// absolute index, record, statistics -- behind the hits of the chunks before, whose number lives in d_counts.  Everything of a chunk runs
// on the caller's stream in chunk order; nothing but the hits is proportional to the number of pairs.
extern "C" int64_t pmx_rect_pairs_count(int64_t nq, int64_t nr)
{
    int64_t total = 0;
    if (nq < 0 || nr < 0) { set_err("negative set size %lld x %lld", (long long)nq, (long long)nr); return -1; }
    if (__builtin_mul_overflow(nq, nr, &total)) { set_err("%lld x %lld pairs overflow 2^63 - 1", (long long)nq, (long long)nr); return -1; }
    return total;
}

// The window [first, first + count) of the rectangle nq x nr: 0, or -1 with the cause.
static int rect_pairs_window(int64_t nq, int64_t nr, int64_t first, int64_t count)
{
    if (first < 0 || count < 0) { set_err("negative first or count"); return -1; }
    const int64_t total = pmx_rect_pairs_count(nq, nr);
    if (total < 0) return -1;
    if (first > total || count > total - first) {
        set_err("pairs %lld .. %lld are beyond the %lld pairs of %lld x %lld sequences", (long long)first, (long long)first + (long long)count - 1,
                (long long)total, (long long)nq, (long long)nr);
        return -1;
    }
    return 0;
}

extern "C" int pmx_rect_pairs_enumerate_device(int64_t nq, int64_t nr, int64_t first, int64_t count, pmx_pair_t *d_pairs, void *stream)
{
    if (rect_pairs_window(nq, nr, first, count)) return -1;
    if (count == 0) return 0;
    if (!d_pairs) { set_err("null pairs"); return -1; }
    const int rc = pmx_launch_rect_pairs_enumerate(nr, first, count, d_pairs, (hipStream_t)stream);
    if (rc) { set_err("pair enumeration launch failed: %s", hipGetErrorString((hipError_t)(-rc))); return rc; }
    return 0;
}

// What both entries refuse about the enumeration.  *R: the reference-side set on return (TRIANGLE: Q).
static int search_pairs_shape_check(const pmx_seqset *Q, const pmx_seqset **R, int shape, int64_t first, int64_t n, const void *pairs)
{
    if (!Q) { set_err("null sequence set"); return -1; }
    if (shape != PMX_PAIRS_LIST && shape != PMX_PAIRS_TRIANGLE && shape != PMX_PAIRS_RECT) { set_err("unknown pair shape %d", shape); return -1; }
    if (shape == PMX_PAIRS_TRIANGLE) {
        if (*R && *R != Q) { set_err("PMX_PAIRS_TRIANGLE takes one set: R must be NULL or Q"); return -1; }
        *R = Q;
    } else if (!*R) { set_err("null sequence set"); return -1; }
    if (first < 0 || n < 0) { set_err("negative first or n"); return -1; }
    if (shape == PMX_PAIRS_LIST) {
        if (first != 0) { set_err("PMX_PAIRS_LIST: first must be 0"); return -1; }
        if (n > 0 && !pairs) { set_err("PMX_PAIRS_LIST: null pairs"); return -1; }
        return 0;
    }
    if (pairs) { set_err("an enumerated shape takes no pair list: pairs must be NULL"); return -1; }
    return shape == PMX_PAIRS_TRIANGLE ? all_pairs_window(Q->count, first, n) : rect_pairs_window(Q->count, (*R)->count, first, n);
}

static int search_pairs_want_check(const pmx_config_t *cfg, bool stats_buffer)
{
    if (cfg->want & PMX_WANT_CIGAR) {
        set_err("set search has no CIGAR output: its hit list is a pair list -- pass the hit pairs to pmx_align_pairs_ex[_device] with PMX_WANT_CIGAR");
        return -1;
    }
    if ((cfg->want & PMX_WANT_STATS) && !stats_buffer) { set_err("stats requested without a stats buffer"); return -1; }
    if (!(cfg->want & PMX_WANT_STATS) && stats_buffer) { set_err("a stats buffer without PMX_WANT_STATS in cfg->want"); return -1; }
    return 0;
}

// The five columns of a hit list, on the device or in a host block: descriptor, absolute index, record, statistics and strand byte
// (nullptr: a column the call does not keep).
struct HitCols {
    pmx_pair_t *pairs; int64_t *index; pmx_record_t *recs; pmx_stats_t *stats; uint8_t *strand;
    void carve(Carver &c, size_t n, bool with_stats, bool with_strand)
    {
        pairs = c.take<pmx_pair_t>(n); index = c.take<int64_t>(n); recs = c.take<pmx_record_t>(n);
        stats = with_stats ? c.take<pmx_stats_t>(n) : nullptr;
        strand = with_strand ? c.take<uint8_t>(n) : nullptr;
    }
};

// The outputs of one run, all device pointers: counts[0] = passing, counts[1] = written; first_bad (host entry over wrapped sets, else
// nullptr) keeps the lowest absolute index of a bad pair.
struct PairHitBufs { HitCols hit; int64_t capacity; int64_t *counts, *first_bad; };

// A chunk's alignment for the entries that keep its records in scratch (set search, top-K): the records (and statistics) of the chunk's
// pairs and, when the entry chooses the strand, those of its alignment slots before the fold and the folded validity bytes.
struct ChunkAlign {
    bool stats; const SlotPlan &plan;
    pmx_record_t *crec = nullptr, *srec = nullptr; pmx_stats_t *cst = nullptr, *sst = nullptr; uint8_t *okf = nullptr;
    ChunkAlign(const pmx_config_t *cfg, const SlotPlan &p) : stats((cfg->want & PMX_WANT_STATS) != 0), plan(p) {}
    void carve(Carver &c, int64_t chunk)
    {
        crec = c.take<pmx_record_t>((size_t)chunk);
        cst = stats ? c.take<pmx_stats_t>((size_t)chunk) : nullptr;
        if (!plan.folds()) return;                              // the slots' records before the fold, the folded validity bytes
        srec = c.take<pmx_record_t>((size_t)chunk * plan.per);
        sst = stats ? c.take<pmx_stats_t>((size_t)chunk * plan.per) : nullptr;
        okf = c.take<uint8_t>((size_t)chunk);
    }
    // The cn pairs of b into crec / cst: a plan without a fold, the alignment and the bad pairs' fix-up; else per * cn slots aligned and
    // folded to cn records that carry their strand or frame.  first_bad != nullptr: the lowest index of a bad pair, the chunk's first pair being p0.
    int run(const pmx_config_t *cfg, const PairsChunkBufs &b, int64_t cn, int32_t max_qlen, int32_t max_rlen, int64_t p0, int64_t *first_bad,
            hipStream_t st) const
    {
        const bool folds = plan.folds();
        int rc = plan.align(cfg, cn * plan.per, b, max_qlen, max_rlen, folds ? srec : crec, folds ? sst : cst, st);
        if (rc) return rc;
        rc = folds ? plan.fold(b, cn, true, srec, sst, crec, cst, nullptr, okf, st) : pmx_launch_pairs_fixup(b.ok, cn, crec, cst, st);
        if (!rc && first_bad) rc = pmx_launch_pairs_first_bad(folds ? okf : b.ok, cn, p0, first_bad, st);
        if (rc) set_err("bad-pair fix-up or strand fold of a chunk failed (%d)", rc);
        return rc;
    }
};

// n > 0 pairs behind the checks; asynchronous on `st`.  index0: the absolute number of the run's first pair (what d_hit_index counts from).
static int search_pairs_run(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int shape, int64_t first, int64_t n,
                            const pmx_pair_t *d_pairs, int64_t index0, int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                            const PairHitBufs &o, hipStream_t st, int64_t chunk, const SlotPlan &plan)
{
    ChunkAlign A(cfg, plan);
    int64_t *cidx = nullptr, *ccnt = nullptr; void *sel = nullptr;
    const size_t sel_bytes = pmx_select_scratch_bytes(chunk, 0, PMX_HITS_BY_INDEX);
    if (scratch_carve(SCR_PSRCH, [&](Carver &c) {
            A.carve(c, chunk);
            cidx = c.take<int64_t>((size_t)chunk); ccnt = c.take<int64_t>(2);
            sel = c.take<unsigned char>(sel_bytes);
        })) return -1;
    HIP_OR_RET(hipMemsetAsync(o.counts, 0, 2 * sizeof(int64_t), st));
    return pairs_run(Q, R, n, d_pairs, first, shape, plan, max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            int rc = A.run(cfg, b, cn, max_qlen, max_rlen, index0 + c0, o.first_bad, st);
            if (rc) return rc;
            rc = pmx_launch_select(A.crec, cn, min_score, 0, PMX_HITS_BY_INDEX, cidx, cn, ccnt, sel, st);
            if (!rc) rc = pmx_launch_pairs_append_hits(cidx, ccnt, cn, o.capacity, index0 + c0, b.pairs, A.crec, A.cst,
                                                       o.hit.pairs, o.hit.index, o.hit.recs, o.hit.stats, o.counts, st, o.hit.strand, plan.marked());
            if (rc) { set_err("hit compaction of a chunk failed (%d)", rc); return rc; }
            return 0;
        });
}

// The side an entry translates, checked and turned into the run's SlotPlan.  TR_NONE: nothing.  TR_QUERY / TR_REF: frame_mode and code.
// TR_CODONS / TR_CODONS_REF (the _frameshift / _frameshift_ref entries): *strand_mode and frameshift; the strands become the run's
// slots, so the mode the pipeline below sees is PMX_STRAND_FORWARD.
static int side_check(const pmx_config_t *cfg, int translated, int frame_mode, const uint8_t *code, int *strand_mode, int32_t frameshift, SlotPlan *fr)
{
    if (translated == TR_NONE) return 0;
    if (translated != TR_CODONS && translated != TR_CODONS_REF) return frames_check(cfg, frame_mode, nullptr, code, fr, translated == TR_REF);
    if (frameshift_check(cfg, *strand_mode, nullptr, frameshift, code, fr, false, translated == TR_CODONS_REF)) return -1;
    *strand_mode = PMX_STRAND_FORWARD;
    return 0;
}

// The device entries; the plain one passes PMX_STRAND_FORWARD and no strand array, and runs what it always ran.  translated (TR_QUERY /
// TR_REF): frame_mode and code of the _translated / _translated_ref entry (strand_mode is then forward, d_hit_strand receives the frames).
static int search_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                               int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                               int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                               pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                               int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts, int strand_mode, uint8_t *d_hit_strand,
                               int translated = TR_NONE, int frame_mode = 0, const uint8_t *code = nullptr, int32_t frameshift = 0)
{
    SlotPlan plan;
    if (search_pairs_shape_check(Q, &R, shape, first, n, d_pairs)) return -1;
    if (capacity < 0) { set_err("negative capacity"); return -1; }
    if (capacity > 0 && !d_hit_recs) { set_err("null hit records with capacity > 0"); return -1; }
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg) || side_check(cfg, translated, frame_mode, code, &strand_mode, frameshift, &plan) ||
        search_pairs_want_check(cfg, d_hit_stats != nullptr) || strand_mode_check(cfg, strand_mode, &plan)) return -1;
    if (byte_out_check(plan, plan.ref && capacity > 0, d_hit_strand)) return -1;       // (only the reference-side entries ask for the column)
    if (n == 0) {
        if (d_counts) HIP_OR_RET(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), (hipStream_t)stream));
        return 0;
    }
    if (!d_counts) { set_err("null counts"); return -1; }
    if (codons_rows_check(plan, max_qlen) || pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_hit_stats != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const PairHitBufs o = {{d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats, d_hit_strand}, capacity, d_counts, nullptr};
    return search_pairs_run(cfg, Q, R, shape, first, n, d_pairs, first, max_qlen, max_rlen, min_score, o, (hipStream_t)stream,
                            pairs_chunk(n, max_qlen, max_rlen, opts, plan.per), plan);
}

extern "C" int pmx_search_pairs_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                       int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                       int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                       pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                       int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, PMX_STRAND_FORWARD, nullptr);
}

extern "C" int pmx_search_pairs_stranded_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                                int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                                int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                                pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                                int strand_mode, uint8_t *d_hit_strand)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, strand_mode, d_hit_strand);
}

extern "C" int pmx_search_pairs_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                                  int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                                  int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                                  pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                  int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                                  int frame_mode, const uint8_t *code, uint8_t *d_hit_frame)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, PMX_STRAND_FORWARD, d_hit_frame, TR_QUERY, frame_mode, code);
}

extern "C" int pmx_search_pairs_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                                      int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                                      int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                                      pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                      int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                                      int frame_mode, const uint8_t *code, uint8_t *d_hit_frame)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, PMX_STRAND_FORWARD, d_hit_frame, TR_REF, frame_mode, code);
}

extern "C" int pmx_search_pairs_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                                  int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                                  int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                                  pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                  int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                                  int strand_mode, uint8_t *d_hit_strand, int32_t frameshift, const uint8_t *code)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, strand_mode, d_hit_strand, TR_CODONS, 0, code, frameshift);
}

extern "C" int pmx_search_pairs_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int shape,
                                                      int64_t first, int64_t n, const pmx_pair_t *d_pairs,
                                                      int32_t max_qlen, int32_t max_rlen, int32_t min_score,
                                                      pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                      int64_t capacity, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts,
                                                      int strand_mode, uint8_t *d_hit_strand, int32_t frameshift, const uint8_t *code)
{
    return search_pairs_device(cfg, Q, R, shape, first, n, d_pairs, max_qlen, max_rlen, min_score, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                               capacity, d_counts, stream, opts, strand_mode, d_hit_strand, TR_CODONS_REF, 0, code, frameshift);
}

extern "C" void pmx_pair_hits_free(pmx_pair_hits_t *hits) { free(hits); }

// The host entries' hit stage: the hits of the slices so far, column by column, until the result block can be sized.
struct HostHits {
    std::vector<pmx_pair_t> pairs; std::vector<int64_t> index; std::vector<pmx_record_t> recs; std::vector<pmx_stats_t> stats; std::vector<uint8_t> strand;
    std::vector<int64_t> row_off, row_passing;                  // top-K: rows + 1 and rows entries; a pair search has none
    int64_t stored = 0, passing = 0;                            // hits held; pairs at or above min_score, held or not
    // the first w hits of a slice's device columns (d.stats / d.strand nullptr: columns the call does not keep) behind those held
    int append(const HitCols &d, int64_t w)
    {
        if (w <= 0) return 0;
        const size_t at = (size_t)stored, n = at + (size_t)w;
        try { pairs.resize(n); index.resize(n); recs.resize(n); if (d.stats) stats.resize(n); if (d.strand) strand.resize(n); }
        catch (const std::bad_alloc &) { set_err("out of memory"); return -1; }
        HIP_OR_RET(hipMemcpy(pairs.data() + at, d.pairs, sizeof(pmx_pair_t) * (size_t)w, hipMemcpyDeviceToHost));
        HIP_OR_RET(hipMemcpy(index.data() + at, d.index, sizeof(int64_t) * (size_t)w, hipMemcpyDeviceToHost));
        HIP_OR_RET(hipMemcpy(recs.data() + at, d.recs, sizeof(pmx_record_t) * (size_t)w, hipMemcpyDeviceToHost));
        if (d.stats) HIP_OR_RET(hipMemcpy(stats.data() + at, d.stats, sizeof(pmx_stats_t) * (size_t)w, hipMemcpyDeviceToHost));
        if (d.strand) HIP_OR_RET(hipMemcpy(strand.data() + at, d.strand, (size_t)w, hipMemcpyDeviceToHost));
        stored += w;
        return 0;
    }
    // The call's result, one zero-filled block released with free(): the header (its size: the result type's; the caller fills it), the
    // row arrays if any, then the descriptors, indices, records, statistics (with_stats) and strand bytes (with_strand) of the hits held,
    // each on a 16-byte boundary, and 16 spare bytes.  *c, *ro, *rp: where the arrays lie.  nullptr: out of memory.
    void *block(size_t header, bool with_stats, bool with_strand, HitCols *c, int64_t **ro = nullptr, int64_t **rp = nullptr) const
    {
        Carver lay; lay.align = 16;
        const size_t h = (size_t)stored, rows = row_passing.size();                 // (no rows: row_off may be empty, the block has its one zero)
        for (int pass = 0; pass < 2; ++pass) {                    // (Carver's two passes: the size, then the block)
            lay.used = 0;
            (void)lay.take<char>(header);
            if (ro) { *ro = lay.take<int64_t>(rows + 1); *rp = lay.take<int64_t>(rows); }
            c->carve(lay, h, with_stats, with_strand);
            if (!lay.base && !(lay.base = (unsigned char *)calloc(1, lay.used + 16))) { set_err("out of memory"); return nullptr; }
        }
        if (ro && rows) { memcpy(*ro, row_off.data(), sizeof(int64_t) * (rows + 1)); memcpy(*rp, row_passing.data(), sizeof(int64_t) * rows); }
        if (h) {
            memcpy(c->pairs, pairs.data(), sizeof(pmx_pair_t) * h); memcpy(c->index, index.data(), sizeof(int64_t) * h);
            memcpy(c->recs, recs.data(), sizeof(pmx_record_t) * h);
            if (with_stats) memcpy(c->stats, stats.data(), sizeof(pmx_stats_t) * h);
            if (with_strand) memcpy(c->strand, strand.data(), h);
        }
        return lay.base;
    }
};

// Both host entries.  with_strand (pmx_search_pairs_stranded): the block is a pmx_strand_hits_t -- the fields of pmx_pair_hits_t, then the
// strand bytes -- and the slices' hit buffers hold one more byte per hit; without it the block and the kernels are pmx_search_pairs'.
// translated (pmx_search_pairs_translated): the block is a pmx_frame_hits_t, the same layout with the frames in the last column; a pair
// without a frame is found on the device only, so the lowest bad pair is always asked for.
static int search_pairs_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                             const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode, bool with_strand, pmx_pair_hits_t **result,
                             int translated = TR_NONE, int frame_mode = 0, const uint8_t *code = nullptr, int32_t frameshift = 0)
{
    SlotPlan plan;
    if (!result) { set_err("null result pointer"); return -1; }
    *result = nullptr;
    if (!opts) { set_err("null opts"); return -1; }
    const int shape = opts->shape;
    const bool listed = shape == PMX_PAIRS_LIST;
    if (search_pairs_shape_check(Q, &R, shape, first, n, pairs)) return -1;
    if (opts->max_hits < 0 || opts->slice_pairs < 0) { set_err("max_hits and slice_pairs must not be negative"); return -1; }
    if (opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg)) return -1;
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    if (side_check(cfg, translated, frame_mode, code, &strand_mode, frameshift, &plan) || search_pairs_want_check(cfg, stats) ||
        strand_mode_check(cfg, strand_mode, &plan)) return -1;
    HostHits hh;
    // the result: one block -- header, descriptors, indices, records, statistics (, strand bytes)
    auto publish = [&]() -> int {
        HitCols c;
        pmx_pair_hits_t *r = (pmx_pair_hits_t *)hh.block(with_strand ? sizeof(pmx_strand_hits_t) : sizeof(pmx_pair_hits_t), stats, with_strand, &c);
        if (!r) return -1;
        r->n_hits = hh.stored; r->n_passing = hh.passing;
        r->pairs = c.pairs; r->index = c.index; r->recs = c.recs; r->stats = c.stats;
        if (with_strand) ((pmx_strand_hits_t *)r)->strand = c.strand;
        *result = r;
        return 0;
    };
    if (n == 0) return publish();
    const bool host_offsets = !Q->h_off.empty() && !R->h_off.empty();
    SetLens m;
    if (host_offsets && listed) {
        const PairScan s = scan_pairs(Q, R, pairs, 0, n);
        if (plan.kind == SlotPlan::CODONS && short_window_check(plan.ref ? R : Q, pairs, s.bad >= 0 ? s.bad : n, plan.ref)) return -1;
        if (s.bad >= 0) { set_err("pair %lld: %s: %s", (long long)s.bad, s.side, s.what); return -1; }
        m.mq = (int32_t)s.mq; m.mr = (int32_t)s.mr; m.mnr = (int32_t)s.mnr;
    } else if (host_offsets && window_host_lens(Q, R, shape, first, n, &m)) return -1;
    auto to_letters = [&]() { plan.to_letters(&m.mq, &m.mr, &m.mnr); };
    to_letters();
    const bool find_bad = !host_offsets || plan.translates();
    const pmx_pairs_opts_t popts = {opts->chunk_pairs};
    if (codons_rows_check(plan, m.mq) || pairs_check(cfg, Q, R, &popts, m.mq, m.mr, stats)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    StreamGuard guard(st);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const pmx_config_t cfg_s = with_sort_hint(cfg, m.mnr, m.mr, n);          // (wrapped sets: no host lengths yet, and no hint from them)
    if (!host_offsets && !listed) {
        if (window_device_lens(cfg, Q, R, &m, st)) return -1;
        to_letters();
    }
    const int64_t slice = std::min<int64_t>(opts->slice_pairs > 0 ? opts->slice_pairs : (int64_t)1 << 24, n);
    const int64_t cap_buf = opts->max_hits > 0 ? std::min<int64_t>(slice, opts->max_hits) : slice;
    HitCols d = {}; pmx_pair_t *dp = nullptr; int64_t *dcnt = nullptr;
    if (scratch_carve(SCR_PHIT, [&](Carver &c) {
            d.carve(c, (size_t)cap_buf, stats, with_strand);
            dcnt = c.take<int64_t>(3);                   // passing, written, first bad pair
        })) return -1;
    if (listed && scratch_reserve(sizeof(pmx_pair_t) * (size_t)slice, (void **)&dp, SCR_PUP)) return -1;
    if (find_bad) HIP_OR_RET(hipMemsetAsync(dcnt + 2, 0xFF, sizeof(int64_t), st));        // (no bad pair yet: the largest unsigned value)
    for (int64_t s0 = 0; s0 < n; s0 += slice) {
        const int64_t sn = std::min<int64_t>(slice, n - s0);
        const int64_t cap = opts->max_hits > 0 ? std::min<int64_t>(sn, opts->max_hits - hh.stored) : sn;
        if (listed) {
            HIP_OR_RET(hipMemcpyAsync(dp, pairs + s0, sizeof(pmx_pair_t) * (size_t)sn, hipMemcpyHostToDevice, st));
            if (!host_offsets) {
                if (device_maxlens(Q, R, dp, sn, &m.mq, &m.mr, st)) return -1;
                to_letters();
                if (pssm_batch_check(cfg->matrix, m.mq, m.mq) || codons_rows_check(plan, m.mq)) return -1;
            }
        }
        const int64_t p0 = listed ? s0 : first + s0;     // the slice's first pair in the enumeration
        const PairHitBufs o = {d, cap, dcnt, find_bad ? dcnt + 2 : nullptr};
        int64_t h[3] = {0, 0, 0};
        int rc = search_pairs_run(&cfg_s, Q, R, shape, listed ? 0 : p0, sn, dp, p0, m.mq, m.mr, opts->min_score, o, st,
                                  pairs_chunk(sn, m.mq, m.mr, &popts, plan.per), plan);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HIP_OR_RET(hipMemcpyAsync(h, dcnt, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipStreamSynchronize(st));
        if (find_bad && h[2] != -1) {
            set_err(plan.translates() ? "pair %lld: bad descriptor (index, window or length) or no frame to translate" : "pair %lld: bad descriptor (index, window or length)",
                    (long long)(h[2] - (listed ? 0 : first)));
            return -1;
        }
        hh.passing += h[0];
        if (hh.append(d, h[1])) return -1;
    }
    return publish();
}

extern "C" int pmx_search_pairs(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, pmx_pair_hits_t **result)
{
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, PMX_STRAND_FORWARD, false, result);
}

extern "C" int pmx_search_pairs_stranded(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                         const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode, pmx_strand_hits_t **result)
{
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, strand_mode, true, (pmx_pair_hits_t **)result);
}
extern "C" void pmx_strand_hits_free(pmx_strand_hits_t *hits) { free(hits); }

extern "C" int pmx_search_pairs_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                           const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int frame_mode, const uint8_t *code,
                                           pmx_frame_hits_t **result)
{
    static_assert(sizeof(pmx_frame_hits_t) == sizeof(pmx_strand_hits_t) && offsetof(pmx_frame_hits_t, frame) == offsetof(pmx_strand_hits_t, strand), "one layout");
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, PMX_STRAND_FORWARD, true, (pmx_pair_hits_t **)result, TR_QUERY, frame_mode, code);
}
extern "C" int pmx_search_pairs_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                               const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int frame_mode, const uint8_t *code,
                                               pmx_frame_hits_t **result)
{
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, PMX_STRAND_FORWARD, true, (pmx_pair_hits_t **)result, TR_REF, frame_mode, code);
}
extern "C" void pmx_frame_hits_free(pmx_frame_hits_t *hits) { free(hits); }
extern "C" int pmx_search_pairs_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                           const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode,
                                           int32_t frameshift, const uint8_t *code, pmx_strand_hits_t **result)
{
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, strand_mode, true, (pmx_pair_hits_t **)result, TR_CODONS, 0, code, frameshift);
}

extern "C" int pmx_search_pairs_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t first, int64_t n,
                                               const pmx_pair_t *pairs, const pmx_pair_search_opts_t *opts, int strand_mode,
                                               int32_t frameshift, const uint8_t *code, pmx_strand_hits_t **result)
{
    return search_pairs_host(cfg, Q, R, first, n, pairs, opts, strand_mode, true, (pmx_pair_hits_t **)result, TR_CODONS_REF, 0, code, frameshift);
}

// ==================================================================== per-query top-K ===
// pmx_search_topk[_device] (semantics: include/parasail_amd.h): the chunk loop of the set batches over whole rows of the
// rectangle Q x R with a body that keeps the chunk's records in scratch and merges them into one list of at most k entries per row
// (pmx_topk.hip); the lists live in scratch until the last chunk, then go to their CSR positions.  Everything of a chunk runs on the
// caller's stream in chunk order.
struct TopkOut { HitCols hit; int64_t capacity; int64_t *row_off, *row_passing, *counts, *first_bad; };

// What both entries refuse about the rows, k and the flag.  *R: the reference-side set on return.
static int topk_shape_check(const pmx_seqset *Q, const pmx_seqset **R, int64_t q_first, int64_t nq, int64_t k, int skip_self)
{
    if (!Q) { set_err("null sequence set"); return -1; }
    if (!*R) *R = Q;
    if (skip_self && *R != Q) { set_err("skip_self needs R to be Q (or NULL): there is no self pair between two sets"); return -1; }
    if (q_first < 0 || nq < 0) { set_err("negative q_first or nq"); return -1; }
    if (q_first > Q->count || nq > Q->count - q_first) {
        set_err("rows %lld .. %lld are beyond the %lld sequences of Q", (long long)q_first, (long long)q_first + (long long)nq - 1, (long long)Q->count);
        return -1;
    }
    if ((*R)->count > INT32_MAX) { set_err("nseq %lld of R is outside 0 .. 2^31 - 1", (long long)(*R)->count); return -1; }
    if (pmx_rect_pairs_count(Q->count, (*R)->count) < 0) return -1;
    if (k < 1 || k > PMX_TOPK_MAX) {
        set_err("k %lld is outside 1 .. %d (a row's list is sorted in LDS): for more hits per query run pmx_search_pairs over the rows and "
                "pmx_select_hits_device per row", (long long)k, PMX_TOPK_MAX);
        return -1;
    }
    return 0;
}

// What the top-K kernels keep between the chunks of a run, shared by topk_run and the record-level hook: the tiles' survivors of one
// chunk, the rows' lists (keys, records, statistics, numbers held, |P_i|) and the scan scratch of the tail.
struct TopkLists {
    int ks = 0; long long rows = 0, tps = 0, tstride = 0;
    uint64_t *tkeys = nullptr, *skeys = nullptr; int32_t *tcnt = nullptr, *tpass = nullptr, *sheld = nullptr; int64_t *spass = nullptr;
    pmx_record_t *srec = nullptr; pmx_stats_t *sst = nullptr; void *scan = nullptr; size_t scan_bytes = 0;
    // ks: min(k, |R|), a row has |R| candidates at most; chunk: the most pairs one merge sees
    void shape(int64_t chunk, int64_t nr, int64_t nq, int32_t k)
    {
        ks = (int)std::min<int64_t>(k, nr);
        pmx_topk_geometry(chunk, nr, ks, &rows, &tps, &tstride);
        scan_bytes = pmx_text_scan_scratch_bytes(nq);
    }
    void carve(Carver &c, int64_t nq, bool stats)
    {
        tkeys = c.take<uint64_t>((size_t)rows * (size_t)tps * (size_t)tstride);
        tcnt = c.take<int32_t>((size_t)rows * (size_t)tps); tpass = c.take<int32_t>((size_t)rows * (size_t)tps);
        skeys = c.take<uint64_t>((size_t)nq * (size_t)ks); srec = c.take<pmx_record_t>((size_t)nq * (size_t)ks);
        sst = stats ? c.take<pmx_stats_t>((size_t)nq * (size_t)ks) : nullptr;
        sheld = c.take<int32_t>((size_t)nq + 2); spass = c.take<int64_t>((size_t)nq);
        scan = c.take<unsigned char>(scan_bytes);
    }
    int clear(int64_t nq, hipStream_t st) const                     // every list empty, before the first chunk
    {
        HIP_OR_RET(hipMemsetAsync(sheld, 0, sizeof(int32_t) * ((size_t)nq + 2), st));
        HIP_OR_RET(hipMemsetAsync(spass, 0, sizeof(int64_t) * (size_t)nq, st));
        return 0;
    }
    // crec / cst: the records (statistics) of pairs [p0, p0 + cn) of the rectangle, p0 absolute
    int merge(const pmx_record_t *crec, const pmx_stats_t *cst, int64_t p0, int64_t cn, int64_t nr, int64_t q_first, int32_t min_score,
              int skip_self, hipStream_t st) const
    {
        const int rc = pmx_launch_topk_merge(crec, cst, p0, cn, nr, q_first, ks, min_score, skip_self, tps, tstride, tkeys, tcnt, tpass,
                                             skeys, srec, sst, sheld, spass, st);
        if (rc) set_err("top-K merge of a chunk failed (%d)", rc);
        return rc;
    }
    // after the last chunk: the rows' offsets, the lists to their CSR positions, the counts
    int finish(int64_t nq, int64_t q_first, int64_t nr, const TopkOut &o, int marked, hipStream_t st) const
    {
        int rc = pmx_launch_text_offsets(sheld, nq, o.row_off, scan, scan_bytes, st);
        if (!rc) rc = pmx_launch_topk_emit(nq, q_first, nr, ks, skeys, srec, sst, sheld, spass, o.row_off, o.capacity, o.hit.pairs, o.hit.index, o.hit.recs, o.hit.stats,
                                           o.row_passing, o.counts, st, o.hit.strand, marked);
        if (rc) { set_err("top-K emit failed (%d)", rc); return rc; }
        return 0;
    }
};
// |R| == 0: no pairs, every row is empty
static int topk_no_pairs(int64_t nq, const TopkOut &o, hipStream_t st)
{
    HIP_OR_RET(hipMemsetAsync(o.row_off, 0, sizeof(int64_t) * (size_t)(nq + 1), st));
    if (o.row_passing) HIP_OR_RET(hipMemsetAsync(o.row_passing, 0, sizeof(int64_t) * (size_t)nq, st));
    HIP_OR_RET(hipMemsetAsync(o.counts, 0, 3 * sizeof(int64_t), st));
    return 0;
}
static const int64_t TOPK_CHUNK_MAX = (int64_t)1 << 26;            // (a chunk's positions fit 32 bits)

// nq > 0 rows behind the checks; asynchronous on `st`.
static int topk_run(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t max_rlen,
                    int32_t min_score, int32_t k, int skip_self, const TopkOut &o, hipStream_t st, const pmx_pairs_opts_t *opts,
                    const SlotPlan &plan)
{
    const int64_t nr = R->count;
    if (nr == 0) return topk_no_pairs(nq, o, st);
    const int64_t n = nq * nr, first = q_first * nr;
    ChunkAlign A(cfg, plan);
    const int64_t chunk = std::min<int64_t>(pairs_chunk(n, max_qlen, max_rlen, opts, plan.per), TOPK_CHUNK_MAX);
    TopkLists L;
    L.shape(chunk, nr, nq, k);
    if (scratch_carve(SCR_PTOPK, [&](Carver &c) { A.carve(c, chunk); L.carve(c, nq, A.stats); })) return -1;
    if (L.clear(nq, st)) return -1;
    int rc = pairs_run(Q, R, n, nullptr, first, PMX_PAIRS_RECT, plan, max_qlen, max_rlen, st, chunk,
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            const int rc = A.run(cfg, b, cn, max_qlen, max_rlen, first + c0, o.first_bad, st);
            return rc ? rc : L.merge(A.crec, A.cst, first + c0, cn, nr, q_first, min_score, skip_self, st);
        });
    if (rc) return rc;
    return L.finish(nq, q_first, nr, o, plan.marked(), st);
}

// Both device entries; the plain one passes PMX_STRAND_FORWARD and no strand array, and runs what it always ran.
static int search_topk_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                              int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                              pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                              int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                              void *stream, const pmx_pairs_opts_t *opts, int strand_mode, uint8_t *d_hit_strand,
                              int translated = TR_NONE, int frame_mode = 0, const uint8_t *code = nullptr, int32_t frameshift = 0)
{
    SlotPlan plan;
    if (topk_shape_check(Q, &R, q_first, nq, k, skip_self)) return -1;
    if (capacity < 0) { set_err("negative capacity"); return -1; }
    if (capacity > 0 && !d_hit_recs) { set_err("null hit records with capacity > 0"); return -1; }
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg) || side_check(cfg, translated, frame_mode, code, &strand_mode, frameshift, &plan) ||
        search_pairs_want_check(cfg, d_hit_stats != nullptr) || strand_mode_check(cfg, strand_mode, &plan)) return -1;
    if (byte_out_check(plan, plan.ref && capacity > 0, d_hit_strand)) return -1;       // (only the reference-side entries ask for the column)
    if (nq == 0) {
        if (d_counts) HIP_OR_RET(hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), (hipStream_t)stream));
        if (d_row_off) HIP_OR_RET(hipMemsetAsync(d_row_off, 0, sizeof(int64_t), (hipStream_t)stream));
        return 0;
    }
    if (!d_row_off) { set_err("null row offsets"); return -1; }
    if (!d_counts) { set_err("null counts"); return -1; }
    if (codons_rows_check(plan, max_qlen) || pairs_check(cfg, Q, R, opts, max_qlen, max_rlen, d_hit_stats != nullptr)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const TopkOut o = {{d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats, d_hit_strand}, capacity, d_row_off, d_row_passing, d_counts, nullptr};
    return topk_run(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, o, (hipStream_t)stream, opts, plan);
}

extern "C" int pmx_search_topk_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                      int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                      pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                      int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                      void *stream, const pmx_pairs_opts_t *opts)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, PMX_STRAND_FORWARD, nullptr);
}

extern "C" int pmx_search_topk_stranded_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                               int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                               pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                               int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                               void *stream, const pmx_pairs_opts_t *opts, int strand_mode, uint8_t *d_hit_strand)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, strand_mode, d_hit_strand);
}

extern "C" int pmx_search_topk_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                                 int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                                 pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                 int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                                 void *stream, const pmx_pairs_opts_t *opts, int frame_mode, const uint8_t *code, uint8_t *d_hit_frame)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, PMX_STRAND_FORWARD, d_hit_frame, TR_QUERY, frame_mode, code);
}

extern "C" int pmx_search_topk_translated_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                                     int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                                     pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                     int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                                     void *stream, const pmx_pairs_opts_t *opts, int frame_mode, const uint8_t *code, uint8_t *d_hit_frame)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, PMX_STRAND_FORWARD, d_hit_frame, TR_REF, frame_mode, code);
}

extern "C" int pmx_search_topk_frameshift_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                                 int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                                 pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                 int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                                 void *stream, const pmx_pairs_opts_t *opts, int strand_mode, uint8_t *d_hit_strand,
                                                 int32_t frameshift, const uint8_t *code)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, strand_mode, d_hit_strand, TR_CODONS, 0, code, frameshift);
}

extern "C" int pmx_search_topk_frameshift_ref_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                                 int32_t max_qlen, int32_t max_rlen, int32_t min_score, int32_t k, int32_t skip_self,
                                                 pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                                 int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts,
                                                 void *stream, const pmx_pairs_opts_t *opts, int strand_mode, uint8_t *d_hit_strand,
                                                 int32_t frameshift, const uint8_t *code)
{
    return search_topk_device(cfg, Q, R, q_first, nq, max_qlen, max_rlen, min_score, k, skip_self, d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats,
                              capacity, d_row_off, d_row_passing, d_counts, stream, opts, strand_mode, d_hit_strand, TR_CODONS_REF, 0, code, frameshift);
}

// Test hook (include/parasail_amd.h): the chunk loop of topk_run over records the caller made up instead of alignments -- the same
// geometry, merges and tail, so scores over all of int32 and rows of any length reach the kernels of pmx_topk.hip.
extern "C" int pmx_topk_records_device(const pmx_record_t *d_rec, const pmx_stats_t *d_stats, int64_t q_first, int64_t nq, int64_t nr,
                                       int32_t min_score, int32_t k, int32_t skip_self, int64_t chunk_pairs,
                                       int32_t marked, uint8_t *d_hit_strand,
                                       pmx_pair_t *d_hit_pairs, int64_t *d_hit_index, pmx_record_t *d_hit_recs, pmx_stats_t *d_hit_stats,
                                       int64_t capacity, int64_t *d_row_off, int64_t *d_row_passing, int64_t *d_counts, void *stream)
{
    int64_t last = 0;
    if (q_first < 0 || nq < 0 || nr < 0) { set_err("negative q_first, nq or nr"); return -1; }
    if (nr > INT32_MAX) { set_err("nr %lld is outside 0 .. 2^31 - 1", (long long)nr); return -1; }
    if (__builtin_add_overflow(q_first, nq, &last) || pmx_rect_pairs_count(last, nr) < 0) {
        set_err("%lld + %lld rows of %lld pairs overflow 2^63 - 1", (long long)q_first, (long long)nq, (long long)nr); return -1;
    }
    if (k < 1 || k > PMX_TOPK_MAX) { set_err("k %lld is outside 1 .. %d (a row's list is sorted in LDS)", (long long)k, PMX_TOPK_MAX); return -1; }
    if (!d_rec) { set_err("null records"); return -1; }
    if (!d_row_off) { set_err("null row offsets"); return -1; }
    if (!d_counts) { set_err("null counts"); return -1; }
    if (capacity < 0) { set_err("negative capacity"); return -1; }
    if (chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (capacity > 0 && !d_hit_recs) { set_err("null hit records with capacity > 0"); return -1; }
    if (d_hit_stats && !d_stats) { set_err("hit statistics without statistics"); return -1; }
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const TopkOut o = {{d_hit_pairs, d_hit_index, d_hit_recs, d_hit_stats, d_hit_strand}, capacity, d_row_off, d_row_passing, d_counts, nullptr};
    if (nq == 0) {
        HIP_OR_RET(hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), st));
        HIP_OR_RET(hipMemsetAsync(d_row_off, 0, sizeof(int64_t), st));
        return 0;
    }
    if (nr == 0) return topk_no_pairs(nq, o, st);
    const int64_t n = nq * nr, first = q_first * nr;
    const int64_t chunk = std::min<int64_t>(std::min<int64_t>(chunk_pairs > 0 ? chunk_pairs : PMX_TOPK_RECORDS_CHUNK, n), TOPK_CHUNK_MAX);
    TopkLists L;
    L.shape(chunk, nr, nq, k);
    if (scratch_carve(SCR_PTOPK, [&](Carver &c) { L.carve(c, nq, d_stats != nullptr); })) return -1;
    if (L.clear(nq, st)) return -1;
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int rc = L.merge(d_rec + c0, d_stats ? d_stats + c0 : nullptr, first + c0, std::min<int64_t>(chunk, n - c0), nr, q_first, min_score,
                               skip_self ? 1 : 0, st);
        if (rc) return rc;
    }
    return L.finish(nq, q_first, nr, o, marked ? 1 : 0, st);
}

extern "C" void pmx_topk_hits_free(pmx_topk_hits_t *hits) { free(hits); }

// Both host entries.  with_strand (pmx_search_topk_stranded): the block is a pmx_topk_strand_hits_t -- the fields of pmx_topk_hits_t, then
// the strand bytes; without it the block and the kernels are pmx_search_topk's.
// translated (pmx_search_topk_translated): a pmx_topk_frame_hits_t, the same layout with the frames in the last column.
static int search_topk_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                            const pmx_topk_opts_t *opts, int strand_mode, bool with_strand, pmx_topk_hits_t **result,
                            int translated = TR_NONE, int frame_mode = 0, const uint8_t *code = nullptr, int32_t frameshift = 0)
{
    SlotPlan plan;
    if (!result) { set_err("null result pointer"); return -1; }
    *result = nullptr;
    if (!opts) { set_err("null opts"); return -1; }
    if (topk_shape_check(Q, &R, q_first, nq, opts->k, opts->skip_self)) return -1;
    if (opts->slice_rows < 0) { set_err("slice_rows must not be negative"); return -1; }
    if (opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg)) return -1;
    const bool stats = (cfg->want & PMX_WANT_STATS) != 0;
    if (side_check(cfg, translated, frame_mode, code, &strand_mode, frameshift, &plan) || search_pairs_want_check(cfg, stats) ||
        strand_mode_check(cfg, strand_mode, &plan)) return -1;
    HostHits hh;
    // the result: one block -- header, row offsets, passing counts, descriptors, indices, records, statistics (, strand bytes)
    auto publish = [&]() -> int {
        HitCols c;
        int64_t *row_off = nullptr, *row_passing = nullptr;
        pmx_topk_hits_t *r = (pmx_topk_hits_t *)hh.block(with_strand ? sizeof(pmx_topk_strand_hits_t) : sizeof(pmx_topk_hits_t), stats, with_strand, &c,
                                                         &row_off, &row_passing);
        if (!r) return -1;
        r->n_rows = nq; r->n_hits = hh.stored; r->n_passing = hh.passing;
        r->row_off = row_off; r->row_passing = row_passing;
        r->pairs = c.pairs; r->index = c.index; r->recs = c.recs; r->stats = c.stats;
        if (with_strand) ((pmx_topk_strand_hits_t *)r)->strand = c.strand;
        *result = r;
        return 0;
    };
    if (nq == 0) return publish();
    const int64_t nr = R->count;
    const bool host_offsets = !Q->h_off.empty() && !R->h_off.empty();
    SetLens m;
    if (host_offsets && nr > 0 && window_host_lens(Q, R, PMX_PAIRS_RECT, q_first * nr, nq * nr, &m)) return -1;
    auto to_letters = [&]() { plan.to_letters(&m.mq, &m.mr, &m.mnr); };
    to_letters();
    const bool find_bad = !host_offsets || plan.translates();
    const pmx_pairs_opts_t popts = {opts->chunk_pairs};
    if (codons_rows_check(plan, m.mq) || pairs_check(cfg, Q, R, &popts, m.mq, m.mr, stats)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    StreamGuard guard(st);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const pmx_config_t cfg_s = with_sort_hint(cfg, m.mnr, m.mr, nq * nr);    // (wrapped sets: no host lengths yet, and no hint from them)
    if (!host_offsets && nr > 0) {
        if (window_device_lens(cfg, Q, R, &m, st)) return -1;
        to_letters();
    }
    // a slice's running state (key, record, statistics per kept entry) stays within the bound of the chunk buffers
    const int64_t ks = std::max<int64_t>(1, std::min<int64_t>(opts->k, nr));
    const int64_t per_row = ks * (int64_t)(8 + sizeof(pmx_record_t) + (stats ? sizeof(pmx_stats_t) : 0)) + 12;
    const int64_t slice = std::min<int64_t>(opts->slice_rows > 0 ? opts->slice_rows : std::max<int64_t>(1, (int64_t)PMX_PAIRS_CHUNK_BYTES / per_row), nq);
    const int64_t cap_buf = slice * ks;
    HitCols d = {}; int64_t *doff = nullptr, *dpass = nullptr, *dcnt = nullptr;
    if (scratch_carve(SCR_PTHIT, [&](Carver &c) {
            d.carve(c, (size_t)cap_buf, stats, with_strand);
            doff = c.take<int64_t>((size_t)slice + 1); dpass = c.take<int64_t>((size_t)slice);
            dcnt = c.take<int64_t>(4);                   // kept, written, passing, first bad pair
        })) return -1;
    if (find_bad) HIP_OR_RET(hipMemsetAsync(dcnt + 3, 0xFF, sizeof(int64_t), st));        // (no bad pair yet: the largest unsigned value)
    try { hh.row_off.assign((size_t)nq + 1, 0); hh.row_passing.assign((size_t)nq, 0); } catch (const std::bad_alloc &) { set_err("out of memory"); return -1; }
    for (int64_t s0 = 0; s0 < nq; s0 += slice) {
        const int64_t sn = std::min<int64_t>(slice, nq - s0);
        const TopkOut o = {d, sn * ks, doff, dpass, dcnt, find_bad ? dcnt + 3 : nullptr};
        int64_t h[4] = {0, 0, 0, 0};
        int rc = topk_run(&cfg_s, Q, R, q_first + s0, sn, m.mq, m.mr, opts->min_score, opts->k, opts->skip_self, o, st, &popts, plan);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HIP_OR_RET(hipMemcpyAsync(h, dcnt, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipStreamSynchronize(st));
        if (find_bad && h[3] != -1) {
            set_err(plan.translates() ? "pair %lld (%lld, %lld): bad descriptor (index, window or length) or no frame to translate"
                       : "pair %lld (%lld, %lld): bad descriptor (index, window or length)", (long long)(h[3] - q_first * nr), (long long)(h[3] / nr), (long long)(h[3] % nr));
            return -1;
        }
        hh.passing += h[2];
        HIP_OR_RET(hipMemcpy(hh.row_off.data() + s0 + 1, doff + 1, sizeof(int64_t) * (size_t)sn, hipMemcpyDeviceToHost));
        HIP_OR_RET(hipMemcpy(hh.row_passing.data() + s0, dpass, sizeof(int64_t) * (size_t)sn, hipMemcpyDeviceToHost));
        for (int64_t x = 1; x <= sn; ++x) hh.row_off[(size_t)(s0 + x)] += hh.stored;
        if (hh.append(d, h[1])) return -1;
    }
    return publish();
}

extern "C" int pmx_search_topk(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                               const pmx_topk_opts_t *opts, pmx_topk_hits_t **result)
{
    return search_topk_host(cfg, Q, R, q_first, nq, opts, PMX_STRAND_FORWARD, false, result);
}

extern "C" int pmx_search_topk_stranded(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                        const pmx_topk_opts_t *opts, int strand_mode, pmx_topk_strand_hits_t **result)
{
    return search_topk_host(cfg, Q, R, q_first, nq, opts, strand_mode, true, (pmx_topk_hits_t **)result);
}
extern "C" void pmx_topk_strand_hits_free(pmx_topk_strand_hits_t *hits) { free(hits); }

extern "C" int pmx_search_topk_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                          const pmx_topk_opts_t *opts, int frame_mode, const uint8_t *code, pmx_topk_frame_hits_t **result)
{
    static_assert(sizeof(pmx_topk_frame_hits_t) == sizeof(pmx_topk_strand_hits_t) && offsetof(pmx_topk_frame_hits_t, frame) == offsetof(pmx_topk_strand_hits_t, strand), "one layout");
    return search_topk_host(cfg, Q, R, q_first, nq, opts, PMX_STRAND_FORWARD, true, (pmx_topk_hits_t **)result, TR_QUERY, frame_mode, code);
}
extern "C" int pmx_search_topk_translated_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                              const pmx_topk_opts_t *opts, int frame_mode, const uint8_t *code, pmx_topk_frame_hits_t **result)
{
    return search_topk_host(cfg, Q, R, q_first, nq, opts, PMX_STRAND_FORWARD, true, (pmx_topk_hits_t **)result, TR_REF, frame_mode, code);
}
extern "C" void pmx_topk_frame_hits_free(pmx_topk_frame_hits_t *hits) { free(hits); }
extern "C" int pmx_search_topk_frameshift(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                          const pmx_topk_opts_t *opts, int strand_mode, int32_t frameshift, const uint8_t *code,
                                          pmx_topk_strand_hits_t **result)
{
    return search_topk_host(cfg, Q, R, q_first, nq, opts, strand_mode, true, (pmx_topk_hits_t **)result, TR_CODONS, 0, code, frameshift);
}

extern "C" int pmx_search_topk_frameshift_ref(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t q_first, int64_t nq,
                                          const pmx_topk_opts_t *opts, int strand_mode, int32_t frameshift, const uint8_t *code,
                                          pmx_topk_strand_hits_t **result)
{
    return search_topk_host(cfg, Q, R, q_first, nq, opts, strand_mode, true, (pmx_topk_hits_t **)result, TR_CODONS_REF, 0, code, frameshift);
}

// ---- k-mer seeding (semantics: include/parasail_amd.h; kernels: pmx_seed.hip) -------------------------------------------
struct pmx_seed_index {
    const pmx_seqset *R = nullptr;
    int k = 0, shift = 0, dev = -1;        // bucket of a key: key >> shift
    int64_t n = 0, nb = 0;                 // entries; buckets (the table holds nb + 1 numbers)
    uint64_t *keys = nullptr, *vals = nullptr; uint32_t *bucket = nullptr;
    int bits = 2;                          // per letter
    int kind = PMX_SEED_KIND_DNA;          // PmxSeedKind: which build made it, and with that which entries seed it
    uint8_t table[256] = {0}; uint8_t *d_table = nullptr;       // letters, translated: the groups and their device copy
    int strands = -2;                      // translated: the PMX_STRAND_* mode it holds; else -2 (what pmx_seed_index_strands answers)
    int w = 1;                             // the window: 1 every k-mer, > 1 a minimizer index (pmx_seed_index_build_minimizers)
    int64_t owned = 0;                     // device bytes behind keys, vals, bucket and d_table
};
static const int PMX_SEED_BUCKET_BITS = 22;            // 2^22 + 1 numbers of 4 bytes: 16 MiB, resident in the Infinity Cache
static const int32_t PMX_SEED_BAND_MAX = 1 << 20;
static thread_local int64_t g_seed_budget = 0;         // the test hook's match buffer; 0: PMX_PAIRS_CHUNK_BYTES
static int64_t seed_match_budget() { return g_seed_budget > 0 ? g_seed_budget : (int64_t)PMX_PAIRS_CHUNK_BYTES; }
extern "C" int64_t pmx_seed_match_budget(int64_t bytes)
{
    const int64_t was = seed_match_budget();
    g_seed_budget = bytes > 0 ? std::min<int64_t>(bytes, (int64_t)1 << 34) : 0;
    return was;
}

extern "C" void pmx_seed_index_free(pmx_seed_index_t *ix)
{
    if (!ix) return;
    if (ix->keys || ix->vals || ix->bucket || ix->d_table) {
        int dev = -1;
        const bool move = hipGetDevice(&dev) == hipSuccess && dev != ix->dev;
        if (move) (void)hipSetDevice(ix->dev);
        (void)hipFree(ix->keys); (void)hipFree(ix->vals); (void)hipFree(ix->bucket); (void)hipFree(ix->d_table);
        if (move) (void)hipSetDevice(dev);
    }
    delete ix;
}

extern "C" int64_t pmx_seed_index_count(const pmx_seed_index_t *ix) { return ix ? ix->n : -1; }
extern "C" int32_t pmx_seed_index_window(const pmx_seed_index_t *ix) { return ix ? ix->w : -1; }
extern "C" int64_t pmx_seed_index_bytes(const pmx_seed_index_t *ix) { return ix ? ix->owned : -1; }

// The index of R behind the entries' checks; table: the 256 groups of a letters or translated index of `bits` bits per letter, NULL:
// the DNA index; translated: tr_strands is the strand mode held, under `code`, one entry slot per byte and strand
static pmx_seed_index_t *seed_index_build(const pmx_seqset_t *R, int kind, int32_t k, int bits, const uint8_t *table, void *stream, int tr_strands = -2,
                                          const uint8_t *code = nullptr)
{
    pmx_seed_index *ix = new (std::nothrow) pmx_seed_index();
    if (!ix) { set_err("out of memory"); return nullptr; }
    ix->R = R; ix->k = k; ix->dev = R->dev; ix->bits = bits; ix->kind = kind; ix->strands = tr_strands;
    if (table) memcpy(ix->table, table, 256);
    const int bbits = std::min(bits * k, PMX_SEED_BUCKET_BITS);
    ix->shift = bits * k - bbits; ix->nb = (int64_t)1 << bbits;
    if (R->bytes == 0 || R->count == 0) return ix;               // nothing to index: no entry, no device memory, no GPU work
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); delete ix; return nullptr; }
    if (R->dev != dev) { set_err("a sequence set of device %d cannot be used on the current device %d", R->dev, dev); delete ix; return nullptr; }
    const hipStream_t st = (hipStream_t)stream;
    const int nstr = tr_strands == PMX_STRAND_BOTH ? 2 : 1;
    const size_t nbytes = (size_t)R->bytes * (size_t)nstr;                  // entry slots
    const size_t temp_bytes = table ? pmx_seed_index_sort_bytes_letters((long long)nbytes, k, bits) : pmx_seed_index_sort_bytes(R->bytes, k);
    uint64_t *kin = nullptr, *vin = nullptr; void *temp = nullptr; unsigned long long *d_n = nullptr, h_n = 0;
    hipError_t e = hipMalloc((void **)&ix->keys, nbytes * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ix->vals, nbytes * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ix->bucket, sizeof(uint32_t) * (size_t)(ix->nb + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&kin, nbytes * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&vin, nbytes * 8);
    if (e == hipSuccess) e = hipMalloc(&temp, temp_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d_n, sizeof h_n);
    if (e == hipSuccess) e = hipMemsetAsync(d_n, 0, sizeof h_n, st);
    if (e == hipSuccess && table) e = hipMalloc((void **)&ix->d_table, 256);
    if (e == hipSuccess && table) e = hipMemcpyAsync(ix->d_table, ix->table, 256, hipMemcpyHostToDevice, st);
    int rc = 0;
    if (e == hipSuccess && kind == PMX_SEED_KIND_TRANSLATED) {
        PmxCodeTable ct;
        if (code) memcpy(ct.v, code, 64); else pmx_genetic_code_host(ct.v);
        rc = pmx_launch_seed_index_translated(R->d_buf, R->d_off, R->count, R->bytes, k, bits, ix->d_table, ct, nstr, tr_strands == PMX_STRAND_REVERSE ? 1 : 0,
                                              kin, vin, ix->keys, ix->vals, temp, temp_bytes, d_n, st);
    } else if (e == hipSuccess && table)
        rc = pmx_launch_seed_index_letters(R->d_buf, R->d_off, R->count, R->bytes, k, bits, ix->d_table, kin, vin, ix->keys, ix->vals, temp, temp_bytes, d_n, st);
    else if (e == hipSuccess)
        rc = pmx_launch_seed_index(R->d_buf, R->d_off, R->count, R->bytes, k, kin, vin, ix->keys, ix->vals, temp, temp_bytes, d_n, st);
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(&h_n, d_n, sizeof h_n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    if (e == hipSuccess && !rc) { ix->n = (int64_t)h_n; rc = pmx_launch_seed_buckets(ix->keys, ix->n, ix->shift, ix->nb, ix->bucket, st); }
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    (void)hipFree(kin); (void)hipFree(vin); (void)hipFree(temp); (void)hipFree(d_n);
    if (e != hipSuccess || rc) {
        set_err("seed index build failed: %s", e != hipSuccess ? hipGetErrorString(e) : "kernel launch");
        pmx_seed_index_free(ix); return nullptr;
    }
    ix->owned = (int64_t)(nbytes * 16 + sizeof(uint32_t) * (size_t)(ix->nb + 1) + (table ? 256 : 0));
    return ix;
}

// what both DNA builds refuse about set and k
static int seed_dna_build_check(const pmx_seqset_t *R, int32_t k)
{
    if (!R) { set_err("null sequence set"); return -1; }
    if (k < 8 || k > 31) { set_err("k %d is outside 8 .. 31", (int)k); return -1; }
    if (R->bytes > INT32_MAX || R->count > INT32_MAX) {
        set_err("a seed index holds a set of at most 2^31 - 1 bytes and sequences (this one: %lld bytes, %lld sequences): index parts of it",
                (long long)R->bytes, (long long)R->count);
        return -1;
    }
    return 0;
}

extern "C" pmx_seed_index_t *pmx_seed_index_build(const pmx_seqset_t *R, int32_t k, void *stream)
{
    if (seed_dna_build_check(R, k)) return nullptr;
    return seed_index_build(R, PMX_SEED_KIND_DNA, k, 2, nullptr, stream);
}

// ---- minimizers (semantics: include/parasail_amd.h; kernels: pmx_seed.hip) -----------------------------------------------
static bool seed_window_valid(int32_t w)
{
    if (w >= 1 && w <= 64) return true;
    set_err("w %d is outside 1 .. 64", (int)w);
    return false;
}

extern "C" uint64_t pmx_seed_mix(uint64_t key, int32_t k) { return k < 8 || k > 31 ? 0 : pmx_seed_mix_bits(key & (((uint64_t)1 << (2 * k)) - 1), (int)k); }

extern "C" void pmx_seed_sketch_shape(int32_t *row_tile, int32_t *set_tile)
{
    int r = 0, s = 0;
    pmx_seed_sketch_tiles(&r, &s);
    if (row_tile) *row_tile = r;
    if (set_tile) *set_tile = s;
}

// Select first, then sort only what was selected: flag bytes from the sketch kernel's set form, their exclusive scan, a scatter of the
// compact (key, val) pairs to the scanned places, rocPRIM's sort of the n entries, the buckets.  Beyond the 5 bytes per byte of the set
// (flags, scan) everything allocated is proportional to n.
extern "C" pmx_seed_index_t *pmx_seed_index_build_minimizers(const pmx_seqset_t *R, int32_t k, int32_t w, void *stream)
{
    if (seed_dna_build_check(R, k) || !seed_window_valid(w)) return nullptr;
    pmx_seed_index *ix = new (std::nothrow) pmx_seed_index();
    if (!ix) { set_err("out of memory"); return nullptr; }
    ix->R = R; ix->k = k; ix->dev = R->dev; ix->w = w;
    const int bbits = std::min(2 * k, PMX_SEED_BUCKET_BITS);
    ix->shift = 2 * k - bbits; ix->nb = (int64_t)1 << bbits;
    if (R->bytes == 0 || R->count == 0) return ix;               // nothing to index: no entry, no device memory, no GPU work
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); delete ix; return nullptr; }
    if (R->dev != dev) { set_err("a sequence set of device %d cannot be used on the current device %d", R->dev, dev); delete ix; return nullptr; }
    const hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)R->bytes, scan_bytes = pmx_seed_sketch_scan_bytes(R->bytes);
    uint8_t *flags = nullptr; uint32_t *at = nullptr, h_n = 0; void *temp = nullptr; uint64_t *kin = nullptr, *vin = nullptr;
    hipError_t e = hipMalloc((void **)&ix->bucket, sizeof(uint32_t) * (size_t)(ix->nb + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&flags, (bytes + 1 + 3) & ~(size_t)3);
    if (e == hipSuccess) e = hipMalloc((void **)&at, sizeof(uint32_t) * (bytes + 1));
    if (e == hipSuccess) e = hipMalloc(&temp, scan_bytes);
    int rc = 0;
    if (e == hipSuccess) rc = pmx_launch_seed_sketch_set(R->d_buf, R->d_off, R->count, R->bytes, k, w, flags, at, temp, scan_bytes, st);
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(&h_n, at + bytes, sizeof h_n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    (void)hipFree(temp); temp = nullptr;
    if (e == hipSuccess && !rc && h_n > 0) {
        const size_t n = h_n, sort_bytes = pmx_seed_index_sort_bytes((long long)n, k);
        e = hipMalloc((void **)&ix->keys, n * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&ix->vals, n * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&kin, n * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&vin, n * 8);
        if (e == hipSuccess) e = hipMalloc(&temp, sort_bytes);
        if (e == hipSuccess)
            rc = pmx_launch_seed_index_selected(R->d_buf, R->d_off, R->count, R->bytes, k, flags, at, (long long)n, kin, vin, ix->keys, ix->vals, temp,
                                                sort_bytes, st);
    }
    if (e == hipSuccess && !rc) { ix->n = (int64_t)h_n; rc = pmx_launch_seed_buckets(ix->keys, ix->n, ix->shift, ix->nb, ix->bucket, st); }
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    (void)hipFree(flags); (void)hipFree(at); (void)hipFree(temp); (void)hipFree(kin); (void)hipFree(vin);
    if (e != hipSuccess || rc) {
        set_err("seed index build failed: %s", e != hipSuccess ? hipGetErrorString(e) : "kernel launch");
        pmx_seed_index_free(ix); return nullptr;
    }
    ix->owned = 16 * ix->n + (int64_t)sizeof(uint32_t) * (ix->nb + 1);
    return ix;
}

// what both sketch entries refuse; > 0: the orientations per row
static int seed_sketch_check(const pmx_seqset *Q, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t k, int32_t w, int strand_mode, const void *flags)
{
    if (!Q) { set_err("null sequence set"); return -1; }
    if (k < 8 || k > 31) { set_err("k %d is outside 8 .. 31", (int)k); return -1; }
    if (!seed_window_valid(w)) return -1;
    if (q_first < 0 || nq < 0) { set_err("negative q_first or nq"); return -1; }
    if (q_first > Q->count || nq > Q->count - q_first) {
        set_err("rows %lld .. %lld are beyond the %lld sequences of Q", (long long)q_first, (long long)q_first + (long long)nq - 1, (long long)Q->count);
        return -1;
    }
    if (strand_mode < PMX_STRAND_FORWARD || strand_mode > PMX_STRAND_BOTH) { set_err("strand mode %d is outside 0 .. 2", strand_mode); return -1; }
    if (max_qlen < 1) { set_err("max_qlen must be positive"); return -1; }
    const int strands = strand_mode == PMX_STRAND_BOTH ? 2 : 1;
    if ((double)nq * strands * ((double)max_qlen + 256.0) > 2147483647.0) {
        set_err("%lld rows x %d strand(s) x max_qlen %d are more than 2^31 - 1 position slots: sketch fewer rows per call", (long long)nq, strands, (int)max_qlen);
        return -1;
    }
    if (nq > 0 && !flags) { set_err("null flags with nq > 0"); return -1; }
    return strands;
}

extern "C" int64_t pmx_seed_rows_max_len(const pmx_seqset_t *Q, int64_t q_first, int64_t nq)
{
    if (!Q) { set_err("null sequence set"); return -1; }
    if (q_first < 0 || nq < 0) { set_err("negative q_first or nq"); return -1; }
    if (q_first > Q->count || nq > Q->count - q_first) {
        set_err("rows %lld .. %lld are beyond the %lld sequences of Q", (long long)q_first, (long long)q_first + (long long)nq - 1, (long long)Q->count);
        return -1;
    }
    if (nq == 0) return 0;
    std::vector<int64_t> copy;
    const int64_t *off = nullptr;
    if (!Q->h_off.empty()) off = Q->h_off.data() + q_first;
    else {                                                   // a wrapped set: its offsets live on the device
        copy.resize((size_t)nq + 1);
        if (hipMemcpy(copy.data(), Q->d_off + q_first, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyDeviceToHost) != hipSuccess) {
            set_err("reading the offsets of a wrapped set failed"); return -1;
        }
        off = copy.data();
    }
    int64_t m = 0;
    for (int64_t r = 0; r < nq; ++r) m = std::max(m, off[r + 1] - off[r]);
    return m;
}

extern "C" int pmx_seed_sketch_device(const pmx_seqset_t *Q, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t k, int32_t w, int strand_mode,
                                      uint8_t *d_flags, void *stream)
{
    const int strands = seed_sketch_check(Q, q_first, nq, max_qlen, k, w, strand_mode, d_flags);
    if (strands < 0) return -1;
    if (nq == 0) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (Q->dev != dev) { set_err("a sequence set of device %d cannot be used on the current device %d", Q->dev, dev); return -1; }
    const int rc = pmx_launch_seed_sketch_rows(Q->d_buf, Q->d_off, Q->bytes, q_first, nq * strands, strands, strand_mode == PMX_STRAND_REVERSE ? 1 : 0, max_qlen,
                                               k, w, d_flags, (hipStream_t)stream);
    if (rc) set_err("seed sketch failed (%d)", rc);
    return rc;
}

extern "C" int pmx_seed_sketch(const pmx_seqset_t *Q, int64_t q_first, int64_t nq, int32_t max_qlen, int32_t k, int32_t w, int strand_mode,
                               uint8_t *flags, void *stream)
{
    const int strands = seed_sketch_check(Q, q_first, nq, max_qlen, k, w, strand_mode, flags);
    if (strands < 0) return -1;
    if (nq == 0) return 0;
    const size_t total = (size_t)nq * (size_t)strands * (size_t)max_qlen;
    uint8_t *d_flags = nullptr;
    if (scratch_reserve(total, (void **)&d_flags, SCR_SEEDHIT)) return -1;
    if (pmx_seed_sketch_device(Q, q_first, nq, max_qlen, k, w, strand_mode, d_flags, stream)) return -1;
    HIP_OR_RET(hipMemcpyAsync(flags, d_flags, total, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_OR_RET(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// The built-in reduced alphabets: one string of letters per group
static const char *const PMX_SEED_AA20[] = {"A", "C", "D", "E", "F", "G", "H", "I", "K", "L", "M", "N", "P", "Q", "R", "S", "T", "V", "W", "Y", nullptr};
static const char *const PMX_SEED_AA11[] = {"KREDQN", "C", "G", "H", "ILV", "M", "F", "Y", "W", "P", "STA", nullptr};

extern "C" int pmx_seed_alphabet(int which, uint8_t table[256])
{
    if (!table) { set_err("null table"); return -1; }
    if (which != PMX_SEED_ALPHABET_AA20 && which != PMX_SEED_ALPHABET_AA11) {
        set_err("alphabet %d is neither PMX_SEED_ALPHABET_AA20 (0) nor PMX_SEED_ALPHABET_AA11 (1)", which); return -1;
    }
    memset(table, 255, 256);
    const char *const *groups = which == PMX_SEED_ALPHABET_AA20 ? PMX_SEED_AA20 : PMX_SEED_AA11;
    for (int g = 0; groups[g]; ++g)
        for (const char *c = groups[g]; *c; ++c) { table[(unsigned char)*c] = (uint8_t)g; table[(unsigned char)*c + 32] = (uint8_t)g; }
    return 0;
}

extern "C" int32_t pmx_seed_index_bits(const pmx_seed_index_t *ix) { return ix ? ix->bits : -1; }

// What the letters and the translated build refuse about set, table and k; > 0: the bits per letter
static int seed_table_bits(const pmx_seqset_t *R, int32_t k, const uint8_t *table)
{
    if (!R) { set_err("null sequence set"); return -1; }
    if (!table) { set_err("null alphabet table"); return -1; }
    int groups = 0;
    for (int b = 0; b < 256; ++b) {
        if (table[b] == 255) continue;
        if (table[b] > 31) { set_err("the alphabet table maps byte %d to group %d: groups are 0 .. 31, 255 marks an invalid byte", b, (int)table[b]); return -1; }
        groups = std::max(groups, (int)table[b] + 1);
    }
    if (groups < 2) { set_err("the alphabet table holds %d group(s): an alphabet has 2 .. 32", groups); return -1; }
    int bits = 1;
    while ((1 << bits) < groups) ++bits;
    if (k < 2 || (int64_t)k * bits > 62) { set_err("k %d with %d bits per letter is outside k >= 2 and k x bits <= 62", (int)k, bits); return -1; }
    return bits;
}

extern "C" pmx_seed_index_t *pmx_seed_index_build_letters(const pmx_seqset_t *R, int32_t k, const uint8_t table[256], void *stream)
{
    const int bits = seed_table_bits(R, k, table);
    if (bits < 0) return nullptr;
    if (R->bytes > ((int64_t)1 << 29) - 1 || R->count > INT32_MAX) {
        set_err("a letters seed index holds a set of at most 2^29 - 1 bytes and 2^31 - 1 sequences (this one: %lld bytes, %lld sequences): index parts of it",
                (long long)R->bytes, (long long)R->count);
        return nullptr;
    }
    return seed_index_build(R, PMX_SEED_KIND_LETTERS, k, bits, table, stream);
}

extern "C" pmx_seed_index_t *pmx_seed_index_build_translated(const pmx_seqset_t *R, int32_t k, const uint8_t table[256], const uint8_t *code,
                                                             int strand_mode, void *stream)
{
    const int bits = seed_table_bits(R, k, table);
    if (bits < 0) return nullptr;
    if (strand_mode < PMX_STRAND_FORWARD || strand_mode > PMX_STRAND_BOTH) { set_err("strand mode %d is outside 0 .. 2", strand_mode); return nullptr; }
    if (R->bytes > ((int64_t)1 << 30) - 1 || R->count > ((int64_t)1 << 29)) {
        set_err("a translated seed index holds a set of at most 2^30 - 1 bytes and 2^29 sequences (this one: %lld bytes, %lld sequences): index parts of it",
                (long long)R->bytes, (long long)R->count);
        return nullptr;
    }
    return seed_index_build(R, PMX_SEED_KIND_TRANSLATED, k, bits, table, stream, strand_mode, code);
}

extern "C" int32_t pmx_seed_index_strands(const pmx_seed_index_t *ix) { return ix ? ix->strands : -1; }

extern "C" int pmx_seed_index_entries_device(const pmx_seed_index_t *ix, int64_t first, int64_t count, uint64_t *d_kmer, int64_t *d_seq,
                                             int32_t *d_pos, void *stream)
{
    if (!ix) { set_err("null seed index"); return -1; }
    if (first < 0 || count < 0) { set_err("negative first or count"); return -1; }
    if (first > ix->n || count > ix->n - first) {
        set_err("entries %lld .. %lld are beyond the %lld entries of the index", (long long)first, (long long)first + (long long)count - 1, (long long)ix->n);
        return -1;
    }
    if (count == 0) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (ix->dev != dev) { set_err("a seed index of device %d cannot be used on the current device %d", ix->dev, dev); return -1; }
    const int rc = pmx_launch_seed_entries(ix->keys, ix->vals, first, count, d_kmer, d_seq, d_pos, (hipStream_t)stream);
    if (rc) set_err("seed index entries failed (%d)", rc);
    return rc;
}

static bool seed_mode_valid(int query_mode) { return query_mode >= PMX_SEED_QUERY_LETTERS && query_mode <= PMX_SEED_CODONS_BOTH; }
// orientation slots per row: the row itself, one frame, three frames (one strand's), six
static int seed_mode_orients(int query_mode)
{
    if (query_mode <= 5) return 1;
    return query_mode == PMX_FRAMES_ALL || query_mode == PMX_SEED_CODONS_BOTH ? 6 : 3;
}

// The one description of a seeding run (pmx_common.h: PmxSeedPlan; host arithmetic only, pinned by tests/test_seed_plans.py).  kind: the
// entry's PmxSeedKind, with its own mode argument behind seed_check -- o.strand (DNA), query_mode (letters: `code` replaces the standard
// genetic code), ref_mode (translated); k, bits, ref_count: the index's; budget: the match buffer in bytes.
// 0 planned; 1 one row's worst case does not fit the budget: the plan is filled up to the slice, which then has no size.
// co: the chain options of pmx_seed_chains[_device] (a DNA index), NULL on the cluster road -- a match then costs what it did.
static int seed_plan(int kind, int mode, const uint8_t *code, int64_t nq, int32_t max_qlen, const pmx_seed_opts_t &o, int k, int bits, int64_t ref_count,
                     int64_t budget, PmxSeedPlan *out, int w = 1, const pmx_seed_chain_opts_t *co = nullptr)
{
    PmxSeedPlan p = {};
    p.kind = kind; p.max_qlen = max_qlen; p.k = k; p.bits = bits; p.ref_count = ref_count; p.w = w;
    p.band = o.band; p.min_seeds = o.min_seeds; p.pad = o.pad; p.max_occ = o.max_occ;
    p.chain = co != nullptr; p.match_bytes = co ? PMX_SEED_MATCH_BYTES_CHAIN : PMX_SEED_MATCH_BYTES;
    if (co) { p.max_gap = co->max_gap; p.lookback = co->lookback; p.gap_scale = co->gap_scale; p.min_score = co->min_score; }
    if (code) memcpy(p.code.v, code, 64); else pmx_genetic_code_host(p.code.v);
    p.orients = p.segs = 1;
    if (kind == PMX_SEED_KIND_DNA) {
        p.geom = PMX_SEED_GEOM_DNA;
        p.orients = p.segs = o.strand == PMX_STRAND_BOTH ? 2 : 1; p.first = o.strand == PMX_STRAND_REVERSE ? 1 : 0;
    } else if (kind == PMX_SEED_KIND_LETTERS) {
        const bool codons = mode >= PMX_SEED_CODONS_FORWARD;
        p.geom = codons ? PMX_SEED_GEOM_CODONS : PMX_SEED_GEOM_FRAMES;
        p.rows_translated = mode != PMX_SEED_QUERY_LETTERS;
        p.orients = seed_mode_orients(mode); p.segs = codons ? p.orients / 3 : p.orients;      // a codon segment is a strand: three frames wide
        p.first = !p.rows_translated ? 0 : mode <= 5 ? mode : mode == PMX_FRAMES_REVERSE || mode == PMX_SEED_CODONS_REVERSE ? 3 : 0;
    } else
        p.geom = mode == PMX_SEED_REF_CODONS ? PMX_SEED_GEOM_REF_CODONS : PMX_SEED_GEOM_REF_FRAMES;       // the rows are proteins: one segment each
    p.row_slots = (int64_t)p.orients * max_qlen; p.seg_slots = p.row_slots / p.segs;
    p.pos_bytes = kind != PMX_SEED_KIND_DNA ? PMX_SEED_POS_BYTES_LETTERS : w > 1 ? PMX_SEED_POS_BYTES_MINIMIZERS : PMX_SEED_POS_BYTES;
    p.key_bits = 33;                                     // the diagonal and the bits of an id: a reference, times the six frames of a translated index
    while (p.key_bits < 64 && ((int64_t)1 << (p.key_bits - 32)) < (kind == PMX_SEED_KIND_TRANSLATED ? 6 : 1) * ref_count) ++p.key_bits;
    *out = p;
    if ((double)p.row_slots * (double)o.max_occ * (double)p.match_bytes > (double)budget) return 1;
    int64_t slice = std::max<int64_t>(1, (int64_t)PMX_PAIRS_CHUNK_BYTES / (p.row_slots * p.pos_bytes));
    if (o.slice_rows > 0) slice = std::min(slice, o.slice_rows);
    slice = std::min(slice, nq);
    // the match buffer: the budget, or the slice's worst case when that is smaller (positions fit 32 bits)
    const double worst = (double)slice * (double)p.row_slots * (double)o.max_occ;
    p.slice_rows = slice; p.positions = slice * p.row_slots; p.slots = slice * p.orients;
    p.cap_m = (int64_t)std::min<double>(std::min<double>((double)(budget / p.match_bytes), worst), 2147483646.0);
    *out = p;
    return 0;
}

/* Test hook (include/parasail_amd.h): the plan with the budget as an argument; no device needed. */
extern "C" int pmx_seed_plan_probe_w(int kind, int mode, long long nq, int max_qlen, int max_occ, long long slice_rows, long long budget,
                                     long long ref_count, int w, long long *out)
{
    if (!out || kind < PMX_SEED_KIND_DNA || kind > PMX_SEED_KIND_TRANSLATED || nq < 1 || max_qlen < 1 || max_occ < 1 || slice_rows < 0 || ref_count < 0) return -1;
    if (w < 1 || w > 64 || (w > 1 && kind != PMX_SEED_KIND_DNA)) return -1;
    pmx_seed_opts_t o = {};
    o.strand = kind == PMX_SEED_KIND_DNA ? mode : 0; o.max_occ = max_occ; o.slice_rows = slice_rows;
    PmxSeedPlan p;
    const int rc = seed_plan(kind, mode, nullptr, nq, max_qlen, o, 0, 0, ref_count, budget > 0 ? std::min<int64_t>(budget, (int64_t)1 << 34) : (int64_t)PMX_PAIRS_CHUNK_BYTES, &p, w);
    const bool oriented = kind == PMX_SEED_KIND_DNA || p.rows_translated;
    const long long v[11] = {p.orients, oriented ? p.first : -1, p.segs, p.seg_slots, p.row_slots, p.pos_bytes, p.slice_rows, p.cap_m, p.positions, p.slots,
                             p.key_bits};
    for (int i = 0; i < 11; ++i) out[i] = rc ? 0 : v[i];
    return rc;
}

extern "C" int pmx_seed_plan_probe(int kind, int mode, long long nq, int max_qlen, int max_occ, long long slice_rows, long long budget,
                                   long long ref_count, long long *out)
{
    return pmx_seed_plan_probe_w(kind, mode, nq, max_qlen, max_occ, slice_rows, budget, ref_count, 1, out);
}

// What the seeding entries refuse about their arguments, and behind that the run's plan.  kind / mode: the entry's (seed_plan); lens_known
// false: the host entry before it has looked at the lengths (max_qlen and the budget rule are checked in its second call).
// chain: the entry is pmx_seed_chains[_device] (kind DNA) and co its chain options, checked behind opts.
static int seed_check(const pmx_seqset *Q, const pmx_seed_index *ix, int kind, int mode, const uint8_t *code, int64_t q_first, int64_t nq, int32_t max_qlen,
                      const pmx_seed_opts_t *o, int64_t capacity, bool lens_known, PmxSeedPlan *plan, bool chain = false,
                      const pmx_seed_chain_opts_t *co = nullptr)
{
    const bool dna = kind == PMX_SEED_KIND_DNA, tref = kind == PMX_SEED_KIND_TRANSLATED, letters = kind == PMX_SEED_KIND_LETTERS;
    if (!lens_known) max_qlen = 1;
    if (!Q) { set_err("null sequence set"); return -1; }
    if (!ix) { set_err("null seed index"); return -1; }
    if (!o) { set_err("null opts"); return -1; }
    if (chain && !co) { set_err("null chain opts"); return -1; }
    if (chain && ix->kind != kind) {
        set_err("chaining takes a DNA index (pmx_seed_index_build, pmx_seed_index_build_minimizers), not a %s one",
                ix->kind == PMX_SEED_KIND_TRANSLATED ? "translated" : "letters");
        return -1;
    }
    if (ix->kind != kind) {
        if (ix->kind == PMX_SEED_KIND_TRANSLATED) set_err("a translated index (pmx_seed_index_build_translated) is seeded by pmx_seed_pairs_translated_ref[_device]");
        else if (ix->kind == PMX_SEED_KIND_LETTERS) set_err("a letters index (pmx_seed_index_build_letters) is seeded by pmx_seed_pairs_letters[_device]");
        else set_err("a DNA index (pmx_seed_index_build) is seeded by pmx_seed_pairs[_device]");
        return -1;
    }
    if (q_first < 0 || nq < 0) { set_err("negative q_first or nq"); return -1; }
    if (capacity < 0) { set_err("negative capacity"); return -1; }
    if (o->max_hits < 0) { set_err("max_hits must not be negative"); return -1; }
    if (o->slice_rows < 0) { set_err("slice_rows must not be negative"); return -1; }
    if (q_first > Q->count || nq > Q->count - q_first) {
        set_err("rows %lld .. %lld are beyond the %lld sequences of Q", (long long)q_first, (long long)q_first + (long long)nq - 1, (long long)Q->count);
        return -1;
    }
    if (max_qlen < 1) { set_err("max_qlen must be positive"); return -1; }
    if (dna && (o->strand < PMX_STRAND_FORWARD || o->strand > PMX_STRAND_BOTH)) { set_err("strand mode %d is outside 0 .. 2", (int)o->strand); return -1; }
    if (tref && o->strand != 0) { set_err("opts->strand %d must be 0 with a translated index: it holds the strands it was built with", (int)o->strand); return -1; }
    if (tref && mode != PMX_SEED_REF_FRAMES && mode != PMX_SEED_REF_CODONS) { set_err("ref_mode is neither PMX_SEED_REF_FRAMES (0) nor PMX_SEED_REF_CODONS (1)"); return -1; }
    if (letters && o->strand != 0) { set_err("opts->strand %d must be 0 with a letters index: query_mode chooses the orientations", (int)o->strand); return -1; }
    if (letters && !seed_mode_valid(mode)) {
        set_err("query mode %d is none of PMX_SEED_QUERY_LETTERS (-1), a frame 0 .. 5, PMX_FRAMES_FORWARD / _REVERSE / _ALL (6 .. 8), "
                "PMX_SEED_CODONS_FORWARD / _REVERSE / _BOTH (9 .. 11)", mode);
        return -1;
    }
    if (o->min_seeds < 1) { set_err("min_seeds %d is below 1", (int)o->min_seeds); return -1; }
    if (o->band < 0 || o->band > PMX_SEED_BAND_MAX) { set_err("band %d is outside 0 .. 2^20", (int)o->band); return -1; }
    if (o->pad < 0 || o->pad > PMX_SEED_BAND_MAX) { set_err("pad %d is outside 0 .. 2^20", (int)o->pad); return -1; }
    if (o->max_occ < 1 || o->max_occ > 65535) { set_err("max_occ %d is outside 1 .. 65535", (int)o->max_occ); return -1; }
    if (o->reserved != 0) { set_err("reserved must be 0"); return -1; }
    if (chain) {
        if (co->max_gap < 1 || co->max_gap > PMX_SEED_BAND_MAX) { set_err("max_gap %d is outside 1 .. 2^20", (int)co->max_gap); return -1; }
        if (co->lookback < 1 || co->lookback > PMX_SEED_CHAIN_RING) { set_err("lookback %d is outside 1 .. %d", (int)co->lookback, PMX_SEED_CHAIN_RING); return -1; }
        if (co->gap_scale < 0 || co->gap_scale > 65535) { set_err("gap_scale %d is outside 0 .. 65535", (int)co->gap_scale); return -1; }
        if (co->min_score < 0) { set_err("min_score %d is negative", (int)co->min_score); return -1; }
        if (co->reserved[0] || co->reserved[1] || co->reserved[2] || co->reserved[3]) { set_err("chain opts: reserved must be 0"); return -1; }
        // f <= 31 x max_qlen has to fit int32 (include/parasail_amd.h, "Arithmetic")
        if (max_qlen > (1 << 26)) { set_err("max_qlen %d is above 2^26: a chain's score would not fit 32 bits", (int)max_qlen); return -1; }
    }
    if (seed_plan(kind, mode, code, nq, max_qlen, *o, ix->k, ix->bits, ix->R->count, seed_match_budget(), plan, ix->w, chain ? co : nullptr)) {
        set_err("one row's worst case of %d positions x %d %s x max_occ %d x %d bytes per match does not fit the match buffer of %lld bytes: "
                "lower max_occ or split the queries", (int)max_qlen, plan->orients, dna ? "strand(s)" : "orientation(s)", (int)o->max_occ,
                plan->match_bytes, (long long)seed_match_budget());
        return -1;
    }
    return 0;
}

static int seed_device_check(const pmx_seqset *Q, const pmx_seed_index *ix)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (Q->dev != dev) { set_err("a sequence set of device %d cannot be used on the current device %d", Q->dev, dev); return -1; }
    if (ix->dev != dev) { set_err("a seed index of device %d cannot be used on the current device %d", ix->dev, dev); return -1; }
    return 0;
}

// nq > 0 rows behind the checks, by their plan.  Synchronises `st` once per slice: the cut is read back.
static int seed_run(const pmx_seqset *Q, const pmx_seed_index *ix, int64_t q_first, int64_t nq, const PmxSeedPlan &p, const PmxSeedOut &out, hipStream_t st)
{
    HIP_OR_RET(hipMemsetAsync(out.counts, 0, 2 * sizeof(int64_t), st));
    if (ix->n == 0) { HIP_OR_RET(hipMemsetAsync(out.row_off, 0, sizeof(int64_t) * (size_t)(nq + 1), st)); return 0; }
    HIP_OR_RET(hipMemsetAsync(out.row_off, 0, sizeof(int64_t), st));
    PmxSeedSlice s = {};
    s.temp_bytes = pmx_seed_temp_bytes(p.positions, p.cap_m, p.slots, p.chain);
    if (scratch_carve(SCR_SEED, [&](Carver &c) {
            s.lo = c.take<uint32_t>((size_t)p.positions); s.cnt = c.take<uint32_t>((size_t)p.positions + 1); s.moff = c.take<int64_t>((size_t)p.positions + 1);
            s.keys_a = c.take<uint64_t>((size_t)p.cap_m); s.keys_b = c.take<uint64_t>((size_t)p.cap_m);
            if (!p.chain) s.head = c.take<uint32_t>((size_t)p.cap_m);
            s.flag = c.take<uint32_t>((size_t)p.cap_m + 1);
            if (p.chain) {
                s.vals_a = c.take<uint32_t>((size_t)p.cap_m); s.vals_b = c.take<uint32_t>((size_t)p.cap_m);
                s.f = c.take<int32_t>((size_t)p.cap_m); s.pred = c.take<int32_t>((size_t)p.cap_m); s.child = c.take<int32_t>((size_t)p.cap_m);
            }
            s.cut = c.take<int64_t>(2); s.temp = c.take<unsigned char>(s.temp_bytes);
            if (p.kind != PMX_SEED_KIND_DNA) s.codes = c.take<uint8_t>((size_t)p.positions);
            if (p.w > 1) s.mflag = c.take<uint8_t>((size_t)p.positions);
        })) return -1;
    const PmxSeedSource src = {ix->keys, ix->vals, ix->bucket, ix->shift, ix->d_table, ix->R->d_off, Q->d_buf, Q->d_off, Q->bytes};
    for (int64_t row = 0; row < nq;) {
        const int64_t rows = std::min<int64_t>(p.slice_rows, nq - row);
        int rc = pmx_launch_seed_count(p, s, src, q_first + row, rows, st);
        if (rc) { set_err("seed count pass failed (%d)", rc); return rc; }
        int64_t h[2] = {0, 0};
        HIP_OR_RET(hipMemcpyAsync(h, s.cut, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipStreamSynchronize(st));
        if (h[0] < 1 || h[0] > rows || h[1] < 0 || h[1] > p.cap_m) { set_err("seed cut of rows %lld .. is inconsistent", (long long)(q_first + row)); return -1; }
        PmxSeedOut part = out;
        part.row_off += row;
        rc = pmx_launch_seed_cluster(p, s, part, src, q_first + row, h[0], h[1], st);
        if (rc) { set_err("seed cluster pass failed (%d)", rc); return rc; }
        row += h[0];
    }
    return 0;
}

// The device entries; kind / mode / code: the public entry's own (seed_plan)
// (chain, copts, d_hit_chains: pmx_seed_chains_device's)
static int seed_pairs_device(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, int32_t max_qlen,
                             const pmx_seed_opts_t *opts, int kind, int mode, const uint8_t *code, pmx_pair_t *d_hit_pairs, uint8_t *d_hit_strand,
                             pmx_seed_hit_t *d_hit_seeds, int64_t capacity, int64_t *d_row_off, int64_t *d_counts, void *stream,
                             bool chain = false, const pmx_seed_chain_opts_t *copts = nullptr, pmx_seed_chain_t *d_hit_chains = nullptr)
{
    PmxSeedPlan plan;
    if (seed_check(Q, ix, kind, mode, code, q_first, nq, max_qlen, opts, capacity, true, &plan, chain, copts)) return -1;
    if (capacity > 0 && (!d_hit_pairs || !d_hit_strand)) { set_err("null hit pairs or strand bytes with capacity > 0"); return -1; }
    if (nq == 0) {
        if (d_counts) HIP_OR_RET(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), (hipStream_t)stream));
        if (d_row_off) HIP_OR_RET(hipMemsetAsync(d_row_off, 0, sizeof(int64_t), (hipStream_t)stream));
        return 0;
    }
    if (!d_row_off) { set_err("null row offsets"); return -1; }
    if (!d_counts) { set_err("null counts"); return -1; }
    if (seed_device_check(Q, ix)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const PmxSeedOut out = {d_hit_pairs, d_hit_strand, d_hit_seeds, capacity, d_row_off, d_counts, d_hit_chains};
    return seed_run(Q, ix, q_first, nq, plan, out, (hipStream_t)stream);
}

extern "C" int pmx_seed_pairs_device(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, int32_t max_qlen,
                                     const pmx_seed_opts_t *opts, pmx_pair_t *d_hit_pairs, uint8_t *d_hit_strand, pmx_seed_hit_t *d_hit_seeds,
                                     int64_t capacity, int64_t *d_row_off, int64_t *d_counts, void *stream)
{
    return seed_pairs_device(Q, ix, q_first, nq, max_qlen, opts, PMX_SEED_KIND_DNA, 0, nullptr, d_hit_pairs, d_hit_strand, d_hit_seeds, capacity, d_row_off,
                             d_counts, stream);
}

extern "C" int pmx_seed_pairs_letters_device(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, int32_t max_qlen,
                                             const pmx_seed_opts_t *opts, int query_mode, const uint8_t *code,
                                             pmx_pair_t *d_hit_pairs, uint8_t *d_hit_byte, pmx_seed_hit_t *d_hit_seeds, int64_t capacity,
                                             int64_t *d_row_off, int64_t *d_counts, void *stream)
{
    return seed_pairs_device(Q, ix, q_first, nq, max_qlen, opts, PMX_SEED_KIND_LETTERS, query_mode, code, d_hit_pairs, d_hit_byte, d_hit_seeds, capacity,
                             d_row_off, d_counts, stream);
}

extern "C" void pmx_seed_hits_free(pmx_seed_hits_t *hits) { free(hits); }

// chain: pmx_seed_chains -- the block's header is a pmx_seed_chained_t (its first member the pmx_seed_hits_t returned here) and the
// chain records lie behind the strand bytes.
static int seed_pairs_host(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, const pmx_seed_opts_t *opts,
                           int kind, int mode, const uint8_t *code, pmx_seed_hits_t **result, bool chain = false,
                           const pmx_seed_chain_opts_t *copts = nullptr)
{
    if (!result) { set_err("null result pointer"); return -1; }
    *result = nullptr;
    PmxSeedPlan plan;                                        // of the ask first; of the run once the longest row is known
    if (seed_check(Q, ix, kind, mode, code, q_first, nq, 0, opts, 0, false, &plan, chain, copts)) return -1;
    // the result: one block -- header, row offsets, descriptors, seed records, strand bytes (and chain records)
    pmx_seed_chain_t *h_chains = nullptr;
    auto block = [&](int64_t stored, int64_t passing) -> pmx_seed_hits_t * {
        Carver c; c.align = 16;
        if (chain) c.take<pmx_seed_chained_t>(1); else c.take<pmx_seed_hits_t>(1);
        c.take<int64_t>((size_t)nq + 1); c.take<pmx_pair_t>((size_t)stored); c.take<pmx_seed_hit_t>((size_t)stored);
        c.take<uint8_t>((size_t)stored);
        if (chain) c.take<pmx_seed_chain_t>((size_t)stored);
        unsigned char *p = (unsigned char *)calloc(1, c.used ? c.used : 16);
        if (!p) { set_err("out of memory"); return nullptr; }
        Carver d; d.align = 16; d.base = p;
        pmx_seed_chained_t *ch = chain ? d.take<pmx_seed_chained_t>(1) : nullptr;
        pmx_seed_hits_t *r = chain ? &ch->hits : d.take<pmx_seed_hits_t>(1);
        r->n_rows = nq; r->n_hits = stored; r->n_passing = passing;
        r->row_off = d.take<int64_t>((size_t)nq + 1); r->pairs = d.take<pmx_pair_t>((size_t)stored);
        r->seeds = d.take<pmx_seed_hit_t>((size_t)stored); r->strand = d.take<uint8_t>((size_t)stored);
        if (chain) h_chains = ch->chains = d.take<pmx_seed_chain_t>((size_t)stored);
        return r;
    };
    if (nq == 0) { *result = block(0, 0); return *result ? 0 : -1; }
    if (seed_device_check(Q, ix)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    StreamGuard guard(st);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    // the longest query of the rows: from the host's offsets, else (a wrapped set) the longest sequence of Q, found on the device
    int32_t mq = 0;
    if (!Q->h_off.empty()) {
        int64_t m = 0;
        for (int64_t r = q_first; r < q_first + nq; ++r) m = std::max(m, Q->h_off[(size_t)r + 1] - Q->h_off[(size_t)r]);
        if (m > INT32_MAX) { set_err("a query of %lld letters is beyond 2^31 - 1", (long long)m); return -1; }
        mq = (int32_t)m;
    } else {
        int32_t *d_m = nullptr, h_m[2] = {0, 0};
        if (scratch_reserve(2 * sizeof(int32_t), (void **)&d_m, SCR_SEEDHIT)) return -1;
        HIP_OR_RET(hipMemsetAsync(d_m, 0, sizeof h_m, st));
        const int rc = pmx_launch_pairs_maxlen(nullptr, Q->count, Q->d_off, Q->count, Q->bytes, Q->d_off, Q->count, Q->bytes, d_m, st);
        if (rc) { set_err("length scan failed (%d)", rc); return rc; }
        HIP_OR_RET(hipMemcpyAsync(h_m, d_m, sizeof h_m, hipMemcpyDeviceToHost, st));
        HIP_OR_RET(hipStreamSynchronize(st));
        mq = h_m[0];
    }
    if (plan.rows_translated) mq /= 3;                       // the letters of the longest translation
    if (mq < 1) mq = 1;
    if (seed_check(Q, ix, kind, mode, code, q_first, nq, mq, opts, 0, true, &plan, chain, copts)) return -1;
    int64_t *d_off = nullptr, *d_cnt = nullptr; pmx_pair_t *d_pairs = nullptr; pmx_seed_hit_t *d_seeds = nullptr; uint8_t *d_strand = nullptr;
    pmx_seed_chain_t *d_chains = nullptr;
    auto carve = [&](int64_t stored) {
        return scratch_carve(SCR_SEEDHIT, [&](Carver &c) {
            d_cnt = c.take<int64_t>(2); d_off = c.take<int64_t>((size_t)nq + 1);
            d_pairs = c.take<pmx_pair_t>((size_t)stored); d_seeds = c.take<pmx_seed_hit_t>((size_t)stored); d_strand = c.take<uint8_t>((size_t)stored);
            if (chain) d_chains = c.take<pmx_seed_chain_t>((size_t)stored);
        });
    };
    // the number of candidates is known only behind a run: room for two per row first (max_hits when that is less), and where more
    // have to be stored a second run with room for exactly those -- the first run's counts are the same either way
    int64_t h[2] = {0, 0};
    int64_t room = 2 * nq + 16;
    if (opts->max_hits > 0) room = std::min(room, opts->max_hits);
    if (carve(room)) return -1;
    int rc = seed_run(Q, ix, q_first, nq, plan, PmxSeedOut{d_pairs, d_strand, d_seeds, room, d_off, d_cnt, d_chains}, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    HIP_OR_RET(hipMemcpyAsync(h, d_cnt, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    const int64_t passing = h[0], stored = opts->max_hits > 0 ? std::min(passing, opts->max_hits) : passing;
    if (stored > room) {
        if (carve(stored)) return -1;
        rc = seed_run(Q, ix, q_first, nq, plan, PmxSeedOut{d_pairs, d_strand, d_seeds, stored, d_off, d_cnt, d_chains}, st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HIP_OR_RET(hipStreamSynchronize(st));
    }
    pmx_seed_hits_t *r = block(stored, passing);
    if (!r) return -1;
    hipError_t e = hipMemcpy(r->row_off, d_off, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && stored > 0) e = hipMemcpy(r->pairs, d_pairs, sizeof(pmx_pair_t) * (size_t)stored, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stored > 0) e = hipMemcpy(r->seeds, d_seeds, sizeof(pmx_seed_hit_t) * (size_t)stored, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stored > 0) e = hipMemcpy(r->strand, d_strand, (size_t)stored, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stored > 0 && chain) e = hipMemcpy(h_chains, d_chains, sizeof(pmx_seed_chain_t) * (size_t)stored, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_err("copying the candidates back failed: %s", hipGetErrorString(e)); free(r); return -1; }
    *result = r;
    return 0;
}

extern "C" int pmx_seed_pairs(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, const pmx_seed_opts_t *opts,
                              pmx_seed_hits_t **result)
{
    return seed_pairs_host(Q, ix, q_first, nq, opts, PMX_SEED_KIND_DNA, 0, nullptr, result);
}

// Chaining: the DNA road with chain options; the hits header is the first member of the chained block.
extern "C" int pmx_seed_chains_device(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, int32_t max_qlen,
                                      const pmx_seed_opts_t *opts, const pmx_seed_chain_opts_t *copts, pmx_pair_t *d_hit_pairs, uint8_t *d_hit_strand,
                                      pmx_seed_hit_t *d_hit_seeds, pmx_seed_chain_t *d_hit_chains, int64_t capacity, int64_t *d_row_off,
                                      int64_t *d_counts, void *stream)
{
    return seed_pairs_device(Q, ix, q_first, nq, max_qlen, opts, PMX_SEED_KIND_DNA, 0, nullptr, d_hit_pairs, d_hit_strand, d_hit_seeds, capacity, d_row_off,
                             d_counts, stream, true, copts, d_hit_chains);
}

extern "C" int pmx_seed_chains(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, const pmx_seed_opts_t *opts,
                               const pmx_seed_chain_opts_t *copts, pmx_seed_chained_t **result)
{
    static_assert(offsetof(pmx_seed_chained_t, hits) == 0, "the chained block starts with its hits");
    if (!result) { set_err("null result pointer"); return -1; }
    pmx_seed_hits_t *hits = nullptr;
    const int rc = seed_pairs_host(Q, ix, q_first, nq, opts, PMX_SEED_KIND_DNA, 0, nullptr, &hits, true, copts);
    *result = (pmx_seed_chained_t *)hits;
    return rc;
}

extern "C" void pmx_seed_chained_free(pmx_seed_chained_t *chained) { free(chained); }

extern "C" int pmx_seed_pairs_letters(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, const pmx_seed_opts_t *opts,
                                      int query_mode, const uint8_t *code, pmx_seed_hits_t **result)
{
    return seed_pairs_host(Q, ix, q_first, nq, opts, PMX_SEED_KIND_LETTERS, query_mode, code, result);
}

extern "C" int pmx_seed_pairs_translated_ref_device(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, int32_t max_qlen,
                                                    const pmx_seed_opts_t *opts, int ref_mode, pmx_pair_t *d_hit_pairs, uint8_t *d_hit_byte,
                                                    pmx_seed_hit_t *d_hit_seeds, int64_t capacity, int64_t *d_row_off, int64_t *d_counts, void *stream)
{
    return seed_pairs_device(Q, ix, q_first, nq, max_qlen, opts, PMX_SEED_KIND_TRANSLATED, ref_mode, nullptr, d_hit_pairs, d_hit_byte, d_hit_seeds, capacity,
                             d_row_off, d_counts, stream);
}

extern "C" int pmx_seed_pairs_translated_ref(const pmx_seqset_t *Q, const pmx_seed_index_t *ix, int64_t q_first, int64_t nq, const pmx_seed_opts_t *opts,
                                             int ref_mode, pmx_seed_hits_t **result)
{
    return seed_pairs_host(Q, ix, q_first, nq, opts, PMX_SEED_KIND_TRANSLATED, ref_mode, nullptr, result);
}

// ---- the ungapped diagonal filter: pmx_seed_ungapped[_device], pmx_seed_filter[_device], and (2.5t) their _translated
// forms over the codon and translated-index lists.  One body per entry shape; `translated` says which of the two kinds `kind` is. ----
extern "C" void pmx_seed_ungapped_shape(int32_t *lanes, int32_t *step)
{
    if (lanes) *lanes = PMX_UNGAP_LANES;
    if (step) *step = PMX_UNGAP_STEP;
}

// What the entries refuse about the list, the configuration and the byte's kind before any GPU work.  out: the record output
// where the entry needs one.  kind: a byte_kind, or (translated) a list_kind.  *plan: the run's slots -- one per candidate, on the
// strand or in the frame of its byte; a list_kind's plan translates one side, as the gather entry the header names for it does.
static int ungap_list_check(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const void *pairs, const void *seeds,
                            const void *out, bool need_out, const uint8_t *d_byte, int kind, bool translated, const uint8_t *code,
                            const pmx_pairs_opts_t *opts, SlotPlan *plan)
{
    if (!Q || !R) { set_err("null sequence set"); return -1; }
    if (n < 0) { set_err("negative n"); return -1; }
    if (n > 0 && (!pairs || (need_out && !out))) { set_err("null pairs or records"); return -1; }
    if (n > 0 && !seeds) { set_err("null seed records: the diagonals of a candidate are in its pmx_seed_hit_t"); return -1; }
    if (opts && opts->chunk_pairs < 0) { set_err("chunk_pairs must not be negative"); return -1; }
    if (check_cfg(cfg)) return -1;
    if (cfg->matrix->type == PARASAIL_MATRIX_TYPE_PSSM) {
        set_err("the ungapped filter takes no PSSM matrix: a profile belongs to one query, a candidate list has many"); return -1;
    }
    if (translated) {
        if (kind != PMX_SEED_LIST_CODONS && kind != PMX_SEED_LIST_REF_FRAMES && kind != PMX_SEED_LIST_REF_CODONS) {
            set_err("unknown list_kind %d (PMX_SEED_LIST_CODONS %d, PMX_SEED_LIST_REF_FRAMES %d, PMX_SEED_LIST_REF_CODONS %d)", kind,
                    PMX_SEED_LIST_CODONS, PMX_SEED_LIST_REF_FRAMES, PMX_SEED_LIST_REF_CODONS);
            return -1;
        }
        plan->kind = kind == PMX_SEED_LIST_REF_FRAMES ? SlotPlan::FRAMES : SlotPlan::CODONS;
        plan->ref = kind != PMX_SEED_LIST_CODONS;
        plan->set_code(code);
        plan->d_byte = d_byte;
        return 0;
    }
    if (kind != PMX_SEED_BYTE_STRAND && kind != PMX_SEED_BYTE_FRAME) {
        set_err("unknown byte_kind %d (PMX_SEED_BYTE_STRAND 0, PMX_SEED_BYTE_FRAME 1)", kind); return -1;
    }
    if (kind == PMX_SEED_BYTE_FRAME) { plan->kind = SlotPlan::FRAMES; plan->set_code(code); }
    else plan->kind = SlotPlan::BYTES;
    plan->d_byte = d_byte;
    return 0;
}
// The kernel form of a plan that ungap_list_check made
static int ungap_form(const SlotPlan &plan)
{
    if (plan.kind == SlotPlan::CODONS) return plan.ref ? PMX_UNGAP_REF_CODONS : PMX_UNGAP_CODONS;
    return plan.kind == SlotPlan::FRAMES && plan.ref ? PMX_UNGAP_REF_FRAMES : PMX_UNGAP_PLAIN;
}
// ... about the maxima: an ungapped score is a sum of at most max_qlen cells and has to be exact in int32.  A translated list's
// longest diagonal: one cell per codon of a stream (its maximum is the stream's W - 2 letters), and never more than the other side's letters.
static int ungap_lens_check(const pmx_config_t *cfg, int32_t max_qlen, int32_t max_rlen, const SlotPlan &plan)
{
    if (max_qlen < 1 || max_rlen < 1) { set_err("max_qlen / max_rlen must be positive"); return -1; }
    const int64_t w = std::max<int64_t>(std::abs((int64_t)cfg->matrix->min), std::abs((int64_t)cfg->matrix->max));
    const int form = ungap_form(plan);
    if (form == PMX_UNGAP_PLAIN) {
        if (w * (int64_t)max_qlen >= ((int64_t)1 << 31)) {
            set_err("max |w| x max_qlen = %lld x %d does not fit int32: the ungapped score would not be exact", (long long)w, (int)max_qlen); return -1;
        }
        return 0;
    }
    const int64_t ql = form == PMX_UNGAP_CODONS ? ((int64_t)max_qlen + 2) / 3 : max_qlen, rl = form == PMX_UNGAP_REF_CODONS ? ((int64_t)max_rlen + 2) / 3 : max_rlen;
    const int64_t cells = std::min(ql, rl);
    if (w * cells >= ((int64_t)1 << 31)) {
        set_err("max |w| x the longest diagonal's cells = %lld x %lld does not fit int32: the ungapped score would not be exact", (long long)w, (long long)cells);
        return -1;
    }
    return 0;
}
// ... about the selection
static int ungap_filter_check(int64_t n, int64_t nq, const void *row_off, const pmx_seed_filter_opts_t *fopts, int64_t capacity, const void *out_row_off,
                              const void *counts)
{
    if (!fopts) { set_err("null filter opts"); return -1; }
    if (fopts->top_n < 0) { set_err("top_n %d is negative (0: no limit)", (int)fopts->top_n); return -1; }
    if (fopts->min_score < 0) { set_err("min_score %d is negative: a candidate passes from score 0 on", (int)fopts->min_score); return -1; }
    if (fopts->reserved[0] || fopts->reserved[1]) { set_err("reserved must be 0"); return -1; }
    if (nq < 0 || capacity < 0) { set_err("negative nq or capacity"); return -1; }
    if (!row_off || !out_row_off) { set_err("null row offsets"); return -1; }
    if (!counts) { set_err("null counts"); return -1; }
    if (n > 0 && nq == 0) { set_err("%lld candidates in no row: the list is the rows' (n = row_off[nq])", (long long)n); return -1; }
    if (n > INT32_MAX || nq > INT32_MAX) { set_err("a list of %lld candidates in %lld rows is beyond 2^31 - 1: filter it in parts of whole rows", (long long)n, (long long)nq); return -1; }
    return 0;
}
static int ungap_device_check(const pmx_seqset *Q, const pmx_seqset *R)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_err("no usable HIP device"); return -1; }
    if (Q->dev != dev || R->dev != dev) {
        set_err("a sequence set of device %d cannot be used on the current device %d", Q->dev != dev ? Q->dev : R->dev, dev); return -1;
    }
    return 0;
}

// The records of the n > 0 candidates behind the checks: every chunk of the set batches' pipeline through pmx_ungapped_kernel in the
// plan's form.  Asynchronous on `st`.
static int ungap_run(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs, const SlotPlan &plan,
                     const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen, pmx_ungapped_t *d_out, hipStream_t st, const pmx_pairs_opts_t *opts)
{
    DevMat dm;
    if (get_devmat(cfg->matrix, &dm)) return -1;
    const int form = ungap_form(plan);
    static const char *const names[] = {"pmx_ungapped_kernel", "pmx_ungapped_kernel<codons>", "pmx_ungapped_kernel<ref_codons>", "pmx_ungapped_kernel<ref_frames>"};
    return pairs_run(Q, R, n, d_pairs, 0, PMX_PAIRS_LIST, plan, max_qlen, max_rlen, st, pairs_chunk(n, max_qlen, max_rlen, opts),
        [&](int64_t c0, int64_t cn, const PairsChunkBufs &b) -> int {
            const int rc = pmx_launch_ungapped(cn, b.q, b.qoff, b.r, b.roff, b.ok, d_pairs + c0, d_seeds + c0, form, R->d_off, b.tw, b.sflag, dm.d,
                                               d_out + c0, st);
            if (rc) { set_err("ungapped filter launch failed (%d)", rc); return rc < 0 ? rc : -1; }
            g_last_kernel = names[form];
            return 0;
        });
}

static int ungap_entry_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                              const pmx_pair_t *d_pairs, const uint8_t *d_byte, int kind, bool translated, const uint8_t *code,
                              const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                              pmx_ungapped_t *d_out, void *stream, const pmx_pairs_opts_t *opts)
{
    SlotPlan plan;
    if (ungap_list_check(cfg, Q, R, n, d_pairs, d_seeds, d_out, true, d_byte, kind, translated, code, opts, &plan) ||
        ungap_lens_check(cfg, max_qlen, max_rlen, plan)) return -1;
    if (n == 0) return 0;
    if (ungap_device_check(Q, R)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    return ungap_run(cfg, Q, R, n, d_pairs, plan, d_seeds, max_qlen, max_rlen, d_out, (hipStream_t)stream, opts);
}
extern "C" int pmx_seed_ungapped_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                        const pmx_pair_t *d_pairs, const uint8_t *d_byte, int byte_kind, const uint8_t *code,
                                        const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                                        pmx_ungapped_t *d_out, void *stream, const pmx_pairs_opts_t *opts)
{
    return ungap_entry_device(cfg, Q, R, n, d_pairs, d_byte, byte_kind, false, code, d_seeds, max_qlen, max_rlen, d_out, stream, opts);
}
extern "C" int pmx_seed_ungapped_translated_device(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                                   const pmx_pair_t *d_pairs, const uint8_t *d_byte, int list_kind, const uint8_t *code,
                                                   const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen,
                                                   pmx_ungapped_t *d_out, void *stream, const pmx_pairs_opts_t *opts)
{
    return ungap_entry_device(cfg, Q, R, n, d_pairs, d_byte, list_kind, true, code, d_seeds, max_qlen, max_rlen, d_out, stream, opts);
}

// The selection behind the checks; d_byte: the list's bytes as the caller gave them (may be NULL).  Asynchronous on `st`.
struct UngapFilterOut { pmx_pair_t *pairs; uint8_t *byte; pmx_seed_hit_t *seeds; pmx_ungapped_t *ungapped; int64_t *source; int64_t capacity, *row_off, *counts; };
static int ungap_filter_run(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, int64_t n, const pmx_pair_t *d_pairs, const SlotPlan &plan,
                            const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen, int64_t nq, const int64_t *d_row_off,
                            const pmx_seed_filter_opts_t &f, const UngapFilterOut &o, hipStream_t st, const pmx_pairs_opts_t *opts)
{
    if (n == 0) {
        HIP_OR_RET(hipMemsetAsync(o.row_off, 0, sizeof(int64_t) * (size_t)(nq + 1), st));
        HIP_OR_RET(hipMemsetAsync(o.counts, 0, 2 * sizeof(int64_t), st));
        return 0;
    }
    pmx_ungapped_t *ung = nullptr; uint64_t *ka = nullptr, *kb = nullptr; uint32_t *flag = nullptr; void *temp = nullptr;
    const size_t temp_bytes = pmx_ungap_select_temp_bytes(n, nq);
    if (scratch_carve(SCR_UNGAP, [&](Carver &c) {
            ung = c.take<pmx_ungapped_t>((size_t)n); flag = c.take<uint32_t>((size_t)n + 1);
            if (f.top_n > 0) { ka = c.take<uint64_t>((size_t)n); kb = c.take<uint64_t>((size_t)n); }
            temp = c.take<unsigned char>(temp_bytes);
        })) return -1;
    int rc = ungap_run(cfg, Q, R, n, d_pairs, plan, d_seeds, max_qlen, max_rlen, ung, st, opts);
    if (rc) return rc;
    rc = pmx_launch_ungap_select(ung, n, d_row_off, nq, f.min_score, f.top_n, d_pairs, plan.d_byte, d_seeds, ka, kb, flag, temp, temp_bytes,
                                 o.pairs, o.byte, o.seeds, o.ungapped, o.source, o.capacity, o.row_off, o.counts, st);
    if (rc) set_err("ungapped selection failed (%d)", rc);
    return rc;
}

#define PMX_UNGAP_FILTER_DEVICE_ARGS(kind_name) \
    const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n, const pmx_pair_t *d_pairs, const uint8_t *d_byte, int kind_name, \
    const uint8_t *code, const pmx_seed_hit_t *d_seeds, int32_t max_qlen, int32_t max_rlen, int64_t nq, const int64_t *d_row_off, \
    const pmx_seed_filter_opts_t *fopts, pmx_pair_t *d_out_pairs, uint8_t *d_out_byte, pmx_seed_hit_t *d_out_seeds, pmx_ungapped_t *d_out_ungapped, \
    int64_t *d_out_source, int64_t capacity, int64_t *d_out_row_off, int64_t *d_counts, void *stream, const pmx_pairs_opts_t *opts
static int ungap_filter_entry_device(PMX_UNGAP_FILTER_DEVICE_ARGS(kind), bool translated)
{
    SlotPlan plan;
    if (ungap_list_check(cfg, Q, R, n, d_pairs, d_seeds, nullptr, false, d_byte, kind, translated, code, opts, &plan) || ungap_lens_check(cfg, max_qlen, max_rlen, plan) ||
        ungap_filter_check(n, nq, d_row_off, fopts, capacity, d_out_row_off, d_counts) || ungap_device_check(Q, R)) return -1;
    StreamGuard guard(stream);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    const UngapFilterOut o = {d_out_pairs, d_out_byte, d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts};
    return ungap_filter_run(cfg, Q, R, n, d_pairs, plan, d_seeds, max_qlen, max_rlen, nq, d_row_off, *fopts, o, (hipStream_t)stream, opts);
}
extern "C" int pmx_seed_filter_device(PMX_UNGAP_FILTER_DEVICE_ARGS(byte_kind))
{
    return ungap_filter_entry_device(cfg, Q, R, n, d_pairs, d_byte, byte_kind, code, d_seeds, max_qlen, max_rlen, nq, d_row_off, fopts, d_out_pairs, d_out_byte,
                                     d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, stream, opts, false);
}
extern "C" int pmx_seed_filter_translated_device(PMX_UNGAP_FILTER_DEVICE_ARGS(list_kind))
{
    return ungap_filter_entry_device(cfg, Q, R, n, d_pairs, d_byte, list_kind, code, d_seeds, max_qlen, max_rlen, nq, d_row_off, fopts, d_out_pairs, d_out_byte,
                                     d_out_seeds, d_out_ungapped, d_out_source, capacity, d_out_row_off, d_counts, stream, opts, true);
}

// The host entries' maxima: the longest good windows of the uploaded list, found on the device (a bad descriptor counts for nothing);
// with frames the letters of the longest translation.
static int ungap_host_lens(const pmx_config_t *cfg, const pmx_seqset *Q, const pmx_seqset *R, const pmx_pair_t *d_pairs, int64_t n, const SlotPlan &plan,
                           int32_t *mq, int32_t *mr, hipStream_t st)
{
    if (device_maxlens(Q, R, d_pairs, n, mq, mr, st)) return -1;
    plan.to_letters(mq, mr);
    return ungap_lens_check(cfg, *mq, *mr, plan);
}

static int ungap_entry_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                            const pmx_pair_t *pairs, const uint8_t *byte, int kind, bool translated, const uint8_t *code,
                            const pmx_seed_hit_t *seeds, pmx_ungapped_t *out, const pmx_pairs_opts_t *opts)
{
    SlotPlan plan;
    if (ungap_list_check(cfg, Q, R, n, pairs, seeds, out, true, byte, kind, translated, code, opts, &plan)) return -1;
    if (n == 0) return 0;
    if (ungap_device_check(Q, R)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    StreamGuard guard(st);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    pmx_pair_t *dp = nullptr; pmx_seed_hit_t *ds = nullptr; uint8_t *db = nullptr; pmx_ungapped_t *du = nullptr;
    if (scratch_carve(SCR_UNGAPHIT, [&](Carver &c) {
            dp = c.take<pmx_pair_t>((size_t)n); ds = c.take<pmx_seed_hit_t>((size_t)n); db = c.take<uint8_t>((size_t)n); du = c.take<pmx_ungapped_t>((size_t)n);
        })) return -1;
    HIP_OR_RET(hipMemcpyAsync(dp, pairs, sizeof(pmx_pair_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OR_RET(hipMemcpyAsync(ds, seeds, sizeof(pmx_seed_hit_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (byte) { HIP_OR_RET(hipMemcpyAsync(db, byte, (size_t)n, hipMemcpyHostToDevice, st)); plan.d_byte = db; }
    int32_t mq = 1, mr = 1;
    if (ungap_host_lens(cfg, Q, R, dp, n, plan, &mq, &mr, st)) return -1;
    const int rc = ungap_run(cfg, Q, R, n, dp, plan, ds, mq, mr, du, st, opts);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    HIP_OR_RET(hipMemcpyAsync(out, du, sizeof(pmx_ungapped_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    return 0;
}
extern "C" int pmx_seed_ungapped(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                 const pmx_pair_t *pairs, const uint8_t *byte, int byte_kind, const uint8_t *code,
                                 const pmx_seed_hit_t *seeds, pmx_ungapped_t *out, const pmx_pairs_opts_t *opts)
{
    return ungap_entry_host(cfg, Q, R, n, pairs, byte, byte_kind, false, code, seeds, out, opts);
}
extern "C" int pmx_seed_ungapped_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, int64_t n,
                                            const pmx_pair_t *pairs, const uint8_t *byte, int list_kind, const uint8_t *code,
                                            const pmx_seed_hit_t *seeds, pmx_ungapped_t *out, const pmx_pairs_opts_t *opts)
{
    return ungap_entry_host(cfg, Q, R, n, pairs, byte, list_kind, true, code, seeds, out, opts);
}

extern "C" void pmx_seed_filtered_free(pmx_seed_filtered_t *result) { free(result); }

static int ungap_filter_entry_host(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, const pmx_seed_hits_t *hits,
                                   int kind, bool translated, const uint8_t *code, const pmx_seed_filter_opts_t *fopts, const pmx_pairs_opts_t *opts,
                                   pmx_seed_filtered_t **result)
{
    if (!result) { set_err("null result pointer"); return -1; }
    *result = nullptr;
    if (!hits) { set_err("null hits"); return -1; }
    if (hits->n_hits < 0 || hits->n_rows < 0) { set_err("negative n_hits or n_rows"); return -1; }
    if (hits->n_hits < hits->n_passing) {
        set_err("a list that max_hits cut (%lld of %lld candidates stored) cannot be filtered: the selection needs every row in full",
                (long long)hits->n_hits, (long long)hits->n_passing);
        return -1;
    }
    const int64_t n = hits->n_hits, nq = hits->n_rows;
    SlotPlan plan;
    if (ungap_list_check(cfg, Q, R, n, hits->pairs, hits->seeds, nullptr, false, hits->strand, kind, translated, code, opts, &plan)) return -1;
    int64_t unused = 0;
    if (ungap_filter_check(n, nq, hits->row_off, fopts, 0, &unused, &unused)) return -1;
    // the result: one block -- header, row offsets, descriptors, seed records, ungapped records, sources, bytes
    auto block = [&](int64_t kept) -> pmx_seed_filtered_t * {
        Carver c; c.align = 16;
        c.take<pmx_seed_filtered_t>(1); c.take<int64_t>((size_t)nq + 1); c.take<pmx_pair_t>((size_t)kept); c.take<pmx_seed_hit_t>((size_t)kept);
        c.take<pmx_ungapped_t>((size_t)kept); c.take<int64_t>((size_t)kept); c.take<uint8_t>((size_t)kept);
        unsigned char *p = (unsigned char *)calloc(1, c.used ? c.used : 16);
        if (!p) { set_err("out of memory"); return nullptr; }
        Carver d; d.align = 16; d.base = p;
        pmx_seed_filtered_t *r = d.take<pmx_seed_filtered_t>(1);
        r->hits.n_rows = nq; r->hits.n_hits = kept; r->hits.n_passing = kept;
        r->hits.row_off = d.take<int64_t>((size_t)nq + 1); r->hits.pairs = d.take<pmx_pair_t>((size_t)kept);
        r->hits.seeds = d.take<pmx_seed_hit_t>((size_t)kept); r->ungapped = d.take<pmx_ungapped_t>((size_t)kept);
        r->source = d.take<int64_t>((size_t)kept); r->hits.strand = d.take<uint8_t>((size_t)kept);
        return r;
    };
    if (n == 0) { *result = block(0); return *result ? 0 : -1; }
    if (ungap_device_check(Q, R)) return -1;
    static thread_local HostStreams hs;
    if (hs.init(false)) return -1;
    const hipStream_t st = hs.comp;
    StreamGuard guard(st);
    if (!guard.ok) { set_err("stream guard failed"); return -1; }
    pmx_pair_t *dp = nullptr, *op = nullptr; pmx_seed_hit_t *ds = nullptr, *os = nullptr; uint8_t *db = nullptr, *ob = nullptr;
    pmx_ungapped_t *ou = nullptr; int64_t *d_off = nullptr, *o_off = nullptr, *o_src = nullptr, *d_cnt = nullptr;
    if (scratch_carve(SCR_UNGAPHIT, [&](Carver &c) {
            dp = c.take<pmx_pair_t>((size_t)n); ds = c.take<pmx_seed_hit_t>((size_t)n); db = c.take<uint8_t>((size_t)n); d_off = c.take<int64_t>((size_t)nq + 1);
            op = c.take<pmx_pair_t>((size_t)n); os = c.take<pmx_seed_hit_t>((size_t)n); ob = c.take<uint8_t>((size_t)n); ou = c.take<pmx_ungapped_t>((size_t)n);
            o_src = c.take<int64_t>((size_t)n); o_off = c.take<int64_t>((size_t)nq + 1); d_cnt = c.take<int64_t>(2);
        })) return -1;
    HIP_OR_RET(hipMemcpyAsync(dp, hits->pairs, sizeof(pmx_pair_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OR_RET(hipMemcpyAsync(ds, hits->seeds, sizeof(pmx_seed_hit_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OR_RET(hipMemcpyAsync(d_off, hits->row_off, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyHostToDevice, st));
    if (hits->strand) { HIP_OR_RET(hipMemcpyAsync(db, hits->strand, (size_t)n, hipMemcpyHostToDevice, st)); plan.d_byte = db; }
    int32_t mq = 1, mr = 1;
    if (ungap_host_lens(cfg, Q, R, dp, n, plan, &mq, &mr, st)) return -1;
    const UngapFilterOut o = {op, ob, os, ou, o_src, n, o_off, d_cnt};
    const int rc = ungap_filter_run(cfg, Q, R, n, dp, plan, ds, mq, mr, nq, d_off, *fopts, o, st, opts);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    int64_t h[2] = {0, 0};
    HIP_OR_RET(hipMemcpyAsync(h, d_cnt, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_OR_RET(hipStreamSynchronize(st));
    const int64_t kept = h[0];
    if (kept < 0 || kept > n || h[1] != kept) { set_err("the selection's counts are inconsistent"); return -1; }
    pmx_seed_filtered_t *r = block(kept);
    if (!r) return -1;
    hipError_t e = hipMemcpy(r->hits.row_off, o_off, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && kept > 0) e = hipMemcpy(r->hits.pairs, op, sizeof(pmx_pair_t) * (size_t)kept, hipMemcpyDeviceToHost);
    if (e == hipSuccess && kept > 0) e = hipMemcpy(r->hits.seeds, os, sizeof(pmx_seed_hit_t) * (size_t)kept, hipMemcpyDeviceToHost);
    if (e == hipSuccess && kept > 0) e = hipMemcpy(r->hits.strand, ob, (size_t)kept, hipMemcpyDeviceToHost);
    if (e == hipSuccess && kept > 0) e = hipMemcpy(r->ungapped, ou, sizeof(pmx_ungapped_t) * (size_t)kept, hipMemcpyDeviceToHost);
    if (e == hipSuccess && kept > 0) e = hipMemcpy(r->source, o_src, sizeof(int64_t) * (size_t)kept, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_err("copying the kept candidates back failed: %s", hipGetErrorString(e)); free(r); return -1; }
    *result = r;
    return 0;
}
extern "C" int pmx_seed_filter(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, const pmx_seed_hits_t *hits,
                               int byte_kind, const uint8_t *code, const pmx_seed_filter_opts_t *fopts, const pmx_pairs_opts_t *opts,
                               pmx_seed_filtered_t **result)
{
    return ungap_filter_entry_host(cfg, Q, R, hits, byte_kind, false, code, fopts, opts, result);
}
extern "C" int pmx_seed_filter_translated(const pmx_config_t *cfg, const pmx_seqset_t *Q, const pmx_seqset_t *R, const pmx_seed_hits_t *hits,
                                          int list_kind, const uint8_t *code, const pmx_seed_filter_opts_t *fopts, const pmx_pairs_opts_t *opts,
                                          pmx_seed_filtered_t **result)
{
    return ungap_filter_entry_host(cfg, Q, R, hits, list_kind, true, code, fopts, opts, result);
}
