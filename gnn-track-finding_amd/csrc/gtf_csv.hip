// gtf_csv.hip -- the event and truth CSVs parsed on the GPU (include/gtf.h: gtf_csv_parse): the
// bytes of one file in device memory -> selected fields as int64 / double device columns in row
// order, what pandas.read_csv (gtf/io.py read_nodes, run_pipeline._scorers) and np.loadtxt
// (read_edges) give on these files, bit for bit, for every field inside the exact domain of
// include/gtf.h; a field outside it is an error bit and the first offending (row, field), never
// a guess.
//
//   count  one block per CHUNK bytes, 16 bytes a thread: the starts of non-blank lines
//   scan   one exclusive sum over the chunk counts: every chunk's first line ordinal
//   parse  the chunk, the byte before it and a halo of one longest row go to LDS; the line
//          starts of the chunk are listed in LDS (one block scan) and thread k walks the k-th
//          one: a line belongs to the chunk it starts in. Its length first (a row that is too
//          long reports only that), then its fields: a sign, the digits in an integer, the
//          point, the exponent; a requested field is stored, the others are only split
//
// The number: M * 10^e or M / 10^-e with M < 2^53 exact and 10^|e| exact (|e| <= 22): one
// correctly rounded fp64 operation, the sign by negation. -ffp-contract=off.
//
// A batch (gtf_csv_parse_ev): K files of one layout in one text buffer, each from a chunk-aligned
// start, so a chunk belongs to one file. The blocks are the files' chunks laid end to end; a block
// finds its file by one search over the K + 1 chunk offsets and then sees that file's bytes alone:
// before its first byte and from its last one on every read gives '\n', in the 16-byte loads, the
// byte before the chunk and the halo alike. The sum over the chunk counts stays global: file e's
// lines are the difference of the sum at its two chunk offsets, its rows those minus skip_lines,
// not below 0, and one small launch and a scan over K between the scan and the parse give row_off.
// A row goes to row_off[e] plus its index in the file; an error goes to its file's record, with the
// row counted inside the file. gtf_csv_parse is the instantiation without tables (EV = false): file
// 0 at offset 0, nothing read.
//
// No atomic but the error word's and the first-error key's, touched only on a violation. Vector
// stores only. One synchronisation, for the counts.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_search.h"

namespace {

using gtf::bad;
using gtf::fail;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int PER = 16;                           // bytes a thread classifies
constexpr int CHUNK = BLOCK * PER;                // 4096
constexpr int MAXROW = GTF_CSV_MAX_ROW_BYTES;
constexpr int HALO = MAXROW + 16;                 // the longest row, its "\r\n", rounded to a load
constexpr int MAXC = GTF_CSV_MAX_COLUMNS;
constexpr int MAXF = GTF_CSV_MAX_FIELDS;
constexpr int MAX_STARTS = CHUNK / 2;             // a row is at least one byte and its newline
static_assert((CHUNK + HALO) % 16 == 0, "the LDS image is filled in 16-byte pieces");

// error kinds: bit k of counts->error is GTF_CSV_ERR_* = 1 << k
enum { K_DIGITS = 0, K_EXPONENT, K_TEXT, K_EMPTY, K_QUOTE, K_SPACE, K_INT_FORM, K_FIELDS, K_ROW_LONG, K_ROWS };
static_assert((1u << K_ROWS) == GTF_CSV_ERR_ROWS && (1u << K_FIELDS) == GTF_CSV_ERR_FIELDS &&
              (1u << K_TEXT) == GTF_CSV_ERR_TEXT, "the kinds are the header's bits");

enum { R_KEY = 0, R_ERR, R_LINES, R_WORDS };      // the result words (uint64 each)

// ev: carved by carve<true> alone. In the one-file instantiation these pointers are null and only
// code under `if constexpr (EV)` (and the batch-only kernel) may read them.
struct Ws {
    unsigned long long* res;   // [R_WORDS]; ev [2 K] the keys, then the error words, by file, and row_off
    unsigned long long *key, *err;   // the first-error key and the error word of file 0
    int32_t *cnt, *sum;        // [n_chunks + 1] line starts per chunk; their exclusive sum
    int32_t *tab;              // ev [3 K + 1] the caller's table: coff, then start, then bytes
    int32_t *coff;             // ev [K + 1] the files' first chunks among the batch's chunks
    int32_t *start, *bytes;    // ev [K] the file's first byte in the text; its size
    int32_t *rows, *row_off;   // ev [K + 1] rows per file; their exclusive sum
    gtf::Scratch cub;
    size_t total;
};

inline int64_t chunks_of(int64_t n_bytes) { return (n_bytes + CHUNK - 1) / CHUNK; }

// n_bytes: the text up to the end of the last file; K: the files of a batch
template <bool EV>
Ws carve(void* base, int64_t n_bytes, int64_t K) {
    Ws w = {};
    gtf::Arena a(base);
    const size_t c1 = (size_t)chunks_of(n_bytes > 0 ? n_bytes : 0) + 1, k = (size_t)K, k1 = k + 1;
    if constexpr (EV) {
        w.res = a.take<unsigned long long>(2 * k + (k1 + 1) / 2);
        w.key = w.res;
        w.err = w.res + k;
        w.row_off = (int32_t*)(w.res + 2 * k);   // (behind the records: one copy brings both back)
        w.rows = a.take<int32_t>(k1);
        w.tab = a.take<int32_t>(3 * k + 1);
        w.coff = w.tab;
        w.start = w.tab + k1;
        w.bytes = w.start + k;
    } else {
        w.res = a.take<unsigned long long>(R_WORDS);
        w.key = w.res + R_KEY;
        w.err = w.res + R_ERR;
    }
    w.cnt = a.take<int32_t>(c1);
    w.sum = a.take<int32_t>(c1);
    w.cub = gtf::CubNeed().scan<int32_t>((int)(c1 > k1 ? c1 : k1)).take(a);
    w.total = a.used();
    return w;
}

struct Parse {
    const uint8_t* text;
    int32_t n, skip, n_fields, max_rows, n_chunks;   // n: one file's bytes (a batch's: w.bytes)
    int32_t K;                 // ev: the files
    uint8_t delim;
    int8_t req[MAXF];          // per field: its column request, or -1
    uint8_t type[MAXC];
    void* out[MAXC];
    Ws w;
};

// One file as a block sees it: its bytes, its size, and which chunk of it the block has.
struct File {
    const uint8_t* text;
    int32_t n, chunk, e;       // chunk: among the file's own; e: the file
};

// The file of block b: one file's, the text itself; a batch's, the one whose chunks hold b (empty
// files take no chunk and are passed over), block-uniform.
template <bool EV>
__device__ __forceinline__ File file_of(const Parse& a, int b) {
    if constexpr (EV) {
        const int e = gtf::segment_of(a.w.coff, a.K, (int32_t)b);
        return File{a.text + a.w.start[e], a.w.bytes[e], b - a.w.coff[e], e};
    } else {
        return File{a.text, a.n, b, 0};
    }
}

// the byte at i of the file; outside it a newline, so the first line starts at 0 and the last one
// ends, whatever lies before and behind the file in the text
__device__ __forceinline__ uint8_t at(const File& f, int64_t i) { return i >= 0 && i < f.n ? f.text[i] : (uint8_t)'\n'; }

// does a non-blank line start on byte c, with `prev` before it and `next` after it
__device__ __forceinline__ bool starts(uint8_t prev, uint8_t c, uint8_t next) {
    return prev == '\n' && c != '\n' && !(c == '\r' && next == '\n');
}

// ---- count: the line starts of every chunk ----
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_count(Parse a) {
    using Reduce = hipcub::BlockReduce<int, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const File f = file_of<EV>(a, blockIdx.x);
    const int64_t i0 = (int64_t)f.chunk * CHUNK + (int64_t)threadIdx.x * PER;
    uint8_t b[PER + 2];
    b[0] = at(f, i0 - 1);
    if (i0 + PER <= f.n) {
        const uint4 v = *(const uint4*)(f.text + i0);   // (text and start are 16-byte aligned, i0 a multiple of 16)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < PER; j++) b[1 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < PER; j++) b[1 + j] = at(f, i0 + j);
    }
    b[PER + 1] = at(f, i0 + PER);
    int c = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) c += (i0 + j < f.n) && starts(b[j], b[j + 1], b[j + 2]);
    const int total = Reduce(tmp).Sum(c);
    if (threadIdx.x == 0) {
        a.w.cnt[blockIdx.x] = total;
        if (blockIdx.x == 0) a.w.cnt[a.n_chunks] = 0;
    }
}

// ---- parse ----
// Where a block's rows go and where their errors are told: file e, whose row r lies at out + r.
struct Dest {
    int32_t e, out;
};

// row: the row's index in its file
__device__ __forceinline__ void report(const Parse& a, const Dest& d, int kind, int row, int field) {
    atomicOr(&a.w.err[d.e], 1ull << kind);                                              // (only on a violation)
    atomicMin(&a.w.key[d.e], ((unsigned long long)(uint32_t)row << 24) | ((unsigned long long)field << 8) | (unsigned)kind);
}

__device__ const double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

enum { F_QUOTE = 1, F_SPACE = 2, F_BAD = 4, F_POINT = 8, F_EXP = 16 };

// one field of the grammar [+-]digits[.digits][(e|E)[+-]digits], byte by byte
struct Field {
    uint64_t m;        // the mantissa's digits as an integer (the first 18)
    int nd, frac, ex;  // mantissa digit characters; those after the point; the written exponent
    int st, flags, len;
    bool neg, eneg;

    __device__ __forceinline__ void reset() {
        m = 0;
        nd = frac = ex = st = flags = len = 0;
        neg = eneg = false;
    }
    __device__ __forceinline__ void digit(int d) {
        if (nd < 18) m = m * 10 + (uint64_t)d;
        nd++;
    }
    __device__ __forceinline__ void eat(uint8_t c) {
        len++;
        if (c == '"') { flags |= F_QUOTE; return; }
        if (c == ' ' || c == '\t') { flags |= F_SPACE; return; }
        const bool dig = c >= '0' && c <= '9', sign = c == '+' || c == '-', e = c == 'e' || c == 'E';
        const int d = c - '0';
        switch (st) {
        case 0:   // nothing yet
        case 1:   // after the sign
            if (dig) { digit(d); st = 2; }
            else if (c == '.') { flags |= F_POINT; st = 3; }
            else if (sign && st == 0) { neg = c == '-'; st = 1; }
            else flags |= F_BAD;
            break;
        case 2:   // the digits before the point
            if (dig) digit(d);
            else if (c == '.') { flags |= F_POINT; st = 3; }
            else if (e) { flags |= F_EXP; st = 4; }
            else flags |= F_BAD;
            break;
        case 3:   // after the point
            if (dig) { digit(d); frac++; }
            else if (e && nd > 0) { flags |= F_EXP; st = 4; }
            else flags |= F_BAD;
            break;
        case 4:   // after e
            if (dig) { ex = d; st = 6; }
            else if (sign) { eneg = c == '-'; st = 5; }
            else flags |= F_BAD;
            break;
        case 5:   // after the exponent's sign
            if (dig) { ex = d; st = 6; }
            else flags |= F_BAD;
            break;
        default:  // the exponent's digits (saturated: far outside the domain either way)
            if (dig) ex = ex < 100000 ? ex * 10 + d : ex;
            else flags |= F_BAD;
        }
    }
    // the field is over: -1 and the value stored, or the kind of its error
    __device__ __forceinline__ int finish(const Parse& a, int q, int row) const {
        if (flags & F_QUOTE) return K_QUOTE;
        if (q < 0) return -1;
        if (len == 0) return K_EMPTY;
        if (flags & F_SPACE) return K_SPACE;
        if ((flags & F_BAD) || !(st == 2 || st == 3 || st == 6) || nd == 0) return K_TEXT;
        if (a.type[q] == GTF_CSV_INT64) {
            if (flags & (F_POINT | F_EXP)) return K_INT_FORM;
            if (nd > 18) return K_DIGITS;
            ((int64_t*)a.out[q])[row] = neg ? -(int64_t)m : (int64_t)m;
            return -1;
        }
        if (nd > 15) return K_DIGITS;
        double v = 0.0;
        if (m != 0) {
            const int e = (eneg ? -ex : ex) - frac;
            if (e > 22 || e < -22) return K_EXPONENT;
            v = e >= 0 ? __dmul_rn((double)m, P10[e]) : __ddiv_rn((double)m, P10[-e]);
        }
        ((double*)a.out[q])[row] = neg ? -v : v;
        return -1;
    }
};

// row: the row's index in its file (d.out + row: in the columns)
__device__ void parse_row(const Parse& a, const Dest& d, const uint8_t* p, int row) {
    // the content: up to the "\n" or "\r\n" (the image ends in newlines, so the walk ends)
    int len = 0;
    for (;; len++) {
        const uint8_t c = p[len];
        if (c == '\n' || (c == '\r' && p[len + 1] == '\n')) break;
        if (len >= MAXROW) {
            report(a, d, K_ROW_LONG, row, 0);
            return;
        }
    }
    Field f;
    f.reset();
    int field = 0;
    for (int pos = 0; pos <= len; pos++) {
        const uint8_t c = p[pos];
        if (pos < len && c != a.delim) {
            f.eat(c);
            continue;
        }
        if (field < a.n_fields) {
            const int k = f.finish(a, a.req[field], d.out + row);
            if (k >= 0) report(a, d, k, row, field);
        } else if (field == a.n_fields) {
            report(a, d, K_FIELDS, row, field);   // the first field too many
        }
        field++;
        f.reset();
    }
    if (field < a.n_fields) report(a, d, K_FIELDS, row, field);   // the first one missing
}

// ---- a batch's rows per file: the lines between the file's two chunk offsets, less the skipped ----
__global__ __launch_bounds__(BLOCK) void k_file_rows(Parse a) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e > a.K) return;
    int rows = 0;
    if (e < a.K) {
        const int c0 = gtf::clampi(a.w.coff[e], 0, a.n_chunks), c1 = gtf::clampi(a.w.coff[e + 1], c0, a.n_chunks);
        rows = a.w.sum[c1] - a.w.sum[c0] - a.skip;
    }
    a.w.rows[e] = rows > 0 ? rows : 0;
}

template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_parse(Parse a) {
    using Scan = hipcub::BlockScan<int, BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ uint4 image[(16 + CHUNK + HALO) / 16];
    __shared__ uint16_t first[MAX_STARTS];
    uint8_t* const s = (uint8_t*)image + 16;   // s[-1]: the byte before the chunk
    const int tid = threadIdx.x;
    const File f = file_of<EV>(a, blockIdx.x);
    const int64_t c0 = (int64_t)f.chunk * CHUNK;
    for (int j = tid * 16; j < CHUNK + HALO; j += BLOCK * 16) {
        if (c0 + j + 16 <= f.n) {
            image[1 + (j >> 4)] = *(const uint4*)(f.text + c0 + j);
        } else {
            for (int k = 0; k < 16; k++) s[j + k] = at(f, c0 + j + k);
        }
    }
    if (tid == 0) s[-1] = at(f, c0 - 1);
    __syncthreads();
    int mine = 0;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int o = tid * PER + j;
        if (c0 + o < f.n && starts(s[o - 1], s[o], s[o + 1])) {
            mask |= 1u << j;
            mine++;
        }
    }
    int before, total;
    Scan(tmp).ExclusiveSum(mine, before, total);
    for (int j = 0; j < PER; j++) {
        if (mask >> j & 1) {
            if (before < MAX_STARTS) first[before] = (uint16_t)(tid * PER + j);
            before++;
        }
    }
    __syncthreads();
    if (total > MAX_STARTS) total = MAX_STARTS;   // (cannot be: two bytes a row)
    // the chunk's first line among its file's; where the file's rows begin in the columns
    int base = a.w.sum[blockIdx.x];
    Dest d = {0, 0};
    if constexpr (EV) {
        base -= a.w.sum[a.w.coff[f.e]];
        d.e = f.e;
        d.out = a.w.row_off[f.e];
    }
    for (int k = tid; k < total; k += BLOCK) {
        const int row = base + k - a.skip;
        if (row < 0) continue;                    // a skipped line (the header)
        if (row >= a.max_rows - d.out) {
            report(a, d, K_ROWS, a.max_rows - d.out > 0 ? a.max_rows - d.out : 0, 0);
            continue;
        }
        parse_row(a, d, s + first[k], row);
    }
    if constexpr (!EV) {
        if (blockIdx.x == 0 && tid == 0) a.w.res[R_LINES] = (unsigned long long)(uint32_t)a.w.sum[a.n_chunks];
    }
}

// What both entry points ask of the layout and the column request, and the request in kernel
// form. 0, or bad()'s status.
template <typename In>
int request(const In* in, Parse& a, const char* who) {
    char m[260];
    auto no = [&](const char* what) {
        snprintf(m, sizeof(m), "%s: %s", who, what);
        return bad(m);
    };
    if (in->n_fields < 1 || in->n_fields > MAXF) return no("n_fields must be in [1, 64]");
    if (in->n_columns < 0 || in->n_columns > MAXC) return no("n_columns must be in [0, 16]");
    const uint8_t d = in->delimiter;
    if ((d >= '0' && d <= '9') || d == '+' || d == '-' || d == '.' || d == 'e' || d == 'E' || d == '"' || d == '\n' ||
        d == '\r' || d == 0)
        return no("the delimiter is a character of the number grammar, a quote, a line end or 0");
    if ((uintptr_t)in->text % 16) return no("text not aligned to 16 bytes");
    for (int f = 0; f < MAXF; f++) a.req[f] = -1;
    for (int c = 0; c < MAXC; c++) {
        a.type[c] = 0;
        a.out[c] = nullptr;
    }
    for (int c = 0; c < in->n_columns; c++) {
        const gtf_csv_column& q = in->columns[c];
        if (q.field < 0 || q.field >= in->n_fields) {
            snprintf(m, sizeof(m), "%s: column %d asks for field %d of %d", who, c, q.field, in->n_fields);
            return bad(m);
        }
        if (q.type != GTF_CSV_INT64 && q.type != GTF_CSV_DOUBLE) return no("a column type that is neither GTF_CSV_INT64 nor GTF_CSV_DOUBLE");
        if (a.req[q.field] >= 0) return no("a field requested twice");
        if (in->max_rows > 0 && !q.out) return no("null output column with max_rows > 0");
        if ((uintptr_t)q.out % 8) return no("output column not aligned to 8 bytes");
        a.req[q.field] = (int8_t)c;
        a.type[c] = (uint8_t)q.type;
        a.out[c] = q.out;
    }
    a.text = (const uint8_t*)in->text;
    a.skip = in->skip_lines; a.n_fields = in->n_fields; a.max_rows = in->max_rows;
    a.delim = d;
    a.n = 0; a.n_chunks = 0; a.K = 0;
    return 0;
}

void clear(gtf_csv_counts* c) {
    c->n_rows = 0;
    c->error = 0;
    c->first_bad_row = c->first_bad_field = -1;
    c->first_bad_error = 0;
    c->pad_ = 0;
}

// the error word and the first-error key of one file into its counts; true when there is an error
bool errors(gtf_csv_counts* c, unsigned long long err, unsigned long long key) {
    c->error = (uint32_t)err;
    if (!c->error) return false;
    c->first_bad_row = (int32_t)(key >> 24);
    c->first_bad_field = (int32_t)((key >> 8) & 0xffff);
    c->first_bad_error = 1u << (key & 0xff);
    return true;
}

// Every launch of a parse, up to the words the entry point brings back. 0, or fail()'s status.
template <bool EV>
int launch(const Parse& a, hipStream_t st, const char* who) {
    const Ws& w = a.w;
    const gtf::Cub cub{w.cub, st};
    hipError_t e;
    const size_t k = EV ? (size_t)a.K : 1;
    if ((e = hipMemsetAsync(w.key, 0xff, 8 * k, st)) != hipSuccess) return fail(who, "memset", e);
    if ((e = hipMemsetAsync(w.err, 0, EV ? 8 * k : 8 * (R_WORDS - 1), st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_count<EV>, dim3(a.n_chunks), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.cnt, w.sum, a.n_chunks + 1)) != hipSuccess) return fail(who, "scan", e);
    if constexpr (EV) {
        hipLaunchKernelGGL(k_file_rows, dim3(gtf::grid(a.K + 1)), dim3(BLOCK), 0, st, a);
        if ((e = cub.scan(w.rows, w.row_off, a.K + 1)) != hipSuccess) return fail(who, "scan files", e);
    }
    hipLaunchKernelGGL(k_parse<EV>, dim3(a.n_chunks), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    return 0;
}

}  // namespace

extern "C" {

size_t gtf_csv_chunk_bytes(void) { return CHUNK; }

size_t gtf_csv_parse_workspace_bytes(int32_t n_bytes) { return carve<false>(nullptr, n_bytes, 0).total; }

size_t gtf_csv_parse_ev_workspace_bytes(int64_t total_bytes, int32_t n_files) {
    return carve<true>(nullptr, total_bytes, n_files > 0 ? n_files : 0).total;
}

int gtf_csv_parse(const gtf_csv_in* in, gtf_csv_counts* counts, void* workspace, size_t workspace_bytes,
                  gtf_stream_t stream) {
    const char* who = "gtf_csv_parse";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_csv_in", "gtf_csv_in")) return rc;
    if (!counts) return bad("gtf_csv_parse: null counts");
    if (in->n_bytes < 0 || in->skip_lines < 0 || in->max_rows < 0) return bad("gtf_csv_parse: negative sizes");
    if (in->n_bytes > INT32_MAX - 2 * (CHUNK + HALO)) return bad("gtf_csv_parse: a text of 2^31 bytes or more");
    if (in->n_bytes > 0 && !in->text) return bad("gtf_csv_parse: null text");
    Parse a;
    if (int rc = request(in, a, who)) return rc;
    clear(counts);
    if (in->n_bytes == 0) return 0;   // no line at all: nothing launched
    if (!workspace || workspace_bytes < gtf_csv_parse_workspace_bytes(in->n_bytes))
        return bad("gtf_csv_parse: workspace smaller than gtf_csv_parse_workspace_bytes");
    a.n = in->n_bytes;
    a.n_chunks = (int32_t)chunks_of(in->n_bytes);
    a.w = carve<false>(workspace, in->n_bytes, 0);
    const Ws& w = a.w;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (int rc = launch<false>(a, st, who)) return rc;
    unsigned long long r[R_WORDS] = {0, 0, 0};
    if ((e = hipMemcpyAsync(r, w.res, sizeof(r), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    const int64_t lines = (int64_t)r[R_LINES], rows = lines > in->skip_lines ? lines - in->skip_lines : 0;
    counts->n_rows = (int32_t)(rows < in->max_rows ? rows : in->max_rows);
    if (errors(counts, r[R_ERR], r[R_KEY])) {
        snprintf(m, sizeof(m), "gtf_csv_parse: outside the exact domain (error bits 0x%x; first: bit 0x%x at row %d, field %d)",
                 counts->error, counts->first_bad_error, counts->first_bad_row, counts->first_bad_field);
        return bad(m);
    }
    return 0;
}

int gtf_csv_parse_ev(const gtf_csv_in_ev* in, gtf_csv_counts* counts, void* workspace, size_t workspace_bytes,
                     gtf_stream_t stream) {
    const char* who = "gtf_csv_parse_ev";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_csv_in_ev", "gtf_csv_in_ev")) return rc;
    const int32_t K = in->n_files;
    if (K < 0 || in->skip_lines < 0 || in->max_rows < 0) return bad("gtf_csv_parse_ev: negative sizes");
    if (K > 0 && (!in->files || !counts)) return bad("gtf_csv_parse_ev: null files or counts with n_files > 0");
    int64_t end = 0, chunks = 0;   // the end of the last file that has bytes; the batch's chunks
    for (int e = 0; e < K; e++) {
        const gtf_csv_file& f = in->files[e];
        const char* what = f.n_bytes < 0                 ? "has a negative size"
                           : f.start < 0 || f.start % CHUNK ? "does not start on a multiple of gtf_csv_chunk_bytes"
                           : f.n_bytes > 0 && f.start < end ? "starts before the end of the file in front of it"
                                                            : nullptr;
        if (what) {
            snprintf(m, sizeof(m), "gtf_csv_parse_ev: file %d %s (start %d, n_bytes %d)", e, what, f.start, f.n_bytes);
            return bad(m);
        }
        if (f.n_bytes == 0) continue;   // takes no chunk, wherever it says it starts
        if ((int64_t)f.start + f.n_bytes > INT32_MAX - 2 * (CHUNK + HALO)) return bad("gtf_csv_parse_ev: a text of 2^31 bytes or more");
        end = (chunks_of((int64_t)f.start + f.n_bytes)) * CHUNK;
        chunks += chunks_of(f.n_bytes);
    }
    if (end > 0 && !in->text) return bad("gtf_csv_parse_ev: null text");
    Parse a;
    if (int rc = request(in, a, who)) return rc;
    if ((uintptr_t)in->row_off % 4) return bad("gtf_csv_parse_ev: row_off not aligned to 4 bytes");
    for (int e = 0; e < K; e++) clear(&counts[e]);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (chunks == 0) {   // no line at all: nothing launched
        if (in->row_off && (e = hipMemsetAsync(in->row_off, 0, 4 * ((size_t)K + 1), st)) != hipSuccess)
            return fail(who, "memset", e);
        return 0;
    }
    if (!workspace || workspace_bytes < gtf_csv_parse_ev_workspace_bytes(end, K))
        return bad("gtf_csv_parse_ev: workspace smaller than gtf_csv_parse_ev_workspace_bytes");
    a.K = K;
    a.n_chunks = (int32_t)chunks;
    a.w = carve<true>(workspace, end, K);
    const Ws& w = a.w;
    // the table: the files' first chunks among the batch's, their starts and sizes
    std::vector<int32_t> tab(3 * (size_t)K + 1);
    int32_t c = 0;
    for (int f = 0; f < K; f++) {
        tab[f] = c;
        tab[K + 1 + f] = in->files[f].n_bytes ? in->files[f].start : 0;
        tab[2 * K + 1 + f] = in->files[f].n_bytes;
        c += (int32_t)chunks_of(in->files[f].n_bytes);
    }
    tab[K] = c;
    const size_t rw = 2 * (size_t)K + ((size_t)K + 2) / 2;   // the records and row_off, in 8-byte words
    std::vector<unsigned long long> r(rw);
    int rc = 0;
    if ((e = hipMemcpyAsync(w.tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, st)) != hipSuccess)
        rc = fail(who, "table", e);
    if (!rc) rc = launch<true>(a, st, who);
    if (!rc && in->row_off &&
        (e = hipMemcpyAsync(in->row_off, w.row_off, 4 * ((size_t)K + 1), hipMemcpyDeviceToDevice, st)) != hipSuccess)
        rc = fail(who, "row_off", e);
    if (!rc && (e = hipMemcpyAsync(r.data(), w.res, 8 * rw, hipMemcpyDeviceToHost, st)) != hipSuccess) rc = fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess && !rc) rc = fail(who, "synchronize", e);   // (the table is read until here)
    if (rc) return rc;
    const int32_t* off = (const int32_t*)(r.data() + 2 * (size_t)K);
    int first = -1;
    for (int f = 0; f < K; f++) {
        const int64_t b = off[f] < in->max_rows ? off[f] : in->max_rows, t = off[f + 1] < in->max_rows ? off[f + 1] : in->max_rows;
        counts[f].n_rows = (int32_t)(t - b);
        if (errors(&counts[f], r[K + f], r[f]) && first < 0) first = f;
    }
    if (first >= 0) {
        const gtf_csv_counts& q = counts[first];
        snprintf(m, sizeof(m),
                 "gtf_csv_parse_ev: file %d: outside the exact domain (error bits 0x%x; first: bit 0x%x at row %d, field %d)", first,
                 q.error, q.first_bad_error, q.first_bad_row, q.first_bad_field);
        return bad(m);
    }
    return 0;
}

}  // extern "C"
