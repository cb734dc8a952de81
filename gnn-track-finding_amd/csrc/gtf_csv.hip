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
// No atomic but the error word's and the first-error key's, touched only on a violation. Vector
// stores only. One synchronisation, for the counts.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_host.h"

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

struct Ws {
    unsigned long long* res;   // [R_WORDS]
    int32_t *cnt, *sum;        // [n_chunks + 1] line starts per chunk; their exclusive sum
    gtf::Scratch cub;
    size_t total;
};

inline int64_t chunks_of(int64_t n_bytes) { return (n_bytes + CHUNK - 1) / CHUNK; }

Ws carve(void* base, int64_t n_bytes) {
    Ws w;
    gtf::Arena a(base);
    const size_t c1 = (size_t)chunks_of(n_bytes > 0 ? n_bytes : 0) + 1;
    w.res = a.take<unsigned long long>(R_WORDS);
    w.cnt = a.take<int32_t>(c1);
    w.sum = a.take<int32_t>(c1);
    w.cub = gtf::CubNeed().scan<int32_t>((int)c1).take(a);
    w.total = a.used();
    return w;
}

struct Parse {
    const uint8_t* text;
    int32_t n, skip, n_fields, max_rows, n_chunks;
    uint8_t delim;
    int8_t req[MAXF];          // per field: its column request, or -1
    uint8_t type[MAXC];
    void* out[MAXC];
    Ws w;
};

// the byte at i; outside the text a newline, so the first line starts at 0 and the last one ends
__device__ __forceinline__ uint8_t at(const Parse& a, int64_t i) { return i >= 0 && i < a.n ? a.text[i] : (uint8_t)'\n'; }

// does a non-blank line start on byte c, with `prev` before it and `next` after it
__device__ __forceinline__ bool starts(uint8_t prev, uint8_t c, uint8_t next) {
    return prev == '\n' && c != '\n' && !(c == '\r' && next == '\n');
}

// ---- count: the line starts of every chunk ----
__global__ __launch_bounds__(BLOCK) void k_count(Parse a) {
    using Reduce = hipcub::BlockReduce<int, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * PER;
    uint8_t b[PER + 2];
    b[0] = at(a, i0 - 1);
    if (i0 + PER <= a.n) {
        const uint4 v = *(const uint4*)(a.text + i0);   // (text is 16-byte aligned, i0 a multiple of 16)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < PER; j++) b[1 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < PER; j++) b[1 + j] = at(a, i0 + j);
    }
    b[PER + 1] = at(a, i0 + PER);
    int c = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) c += (i0 + j < a.n) && starts(b[j], b[j + 1], b[j + 2]);
    const int total = Reduce(tmp).Sum(c);
    if (threadIdx.x == 0) {
        a.w.cnt[blockIdx.x] = total;
        if (blockIdx.x == 0) a.w.cnt[a.n_chunks] = 0;
    }
}

// ---- parse ----
__device__ __forceinline__ void report(const Parse& a, int kind, int row, int field) {
    atomicOr((unsigned long long*)&a.w.res[R_ERR], 1ull << kind);                       // (only on a violation)
    atomicMin(&a.w.res[R_KEY], ((unsigned long long)(uint32_t)row << 24) | ((unsigned long long)field << 8) | (unsigned)kind);
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

__device__ void parse_row(const Parse& a, const uint8_t* p, int row) {
    // the content: up to the "\n" or "\r\n" (the image ends in newlines, so the walk ends)
    int len = 0;
    for (;; len++) {
        const uint8_t c = p[len];
        if (c == '\n' || (c == '\r' && p[len + 1] == '\n')) break;
        if (len >= MAXROW) {
            report(a, K_ROW_LONG, row, 0);
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
            const int k = f.finish(a, a.req[field], row);
            if (k >= 0) report(a, k, row, field);
        } else if (field == a.n_fields) {
            report(a, K_FIELDS, row, field);   // the first field too many
        }
        field++;
        f.reset();
    }
    if (field < a.n_fields) report(a, K_FIELDS, row, field);   // the first one missing
}

__global__ __launch_bounds__(BLOCK) void k_parse(Parse a) {
    using Scan = hipcub::BlockScan<int, BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ uint4 image[(16 + CHUNK + HALO) / 16];
    __shared__ uint16_t first[MAX_STARTS];
    uint8_t* const s = (uint8_t*)image + 16;   // s[-1]: the byte before the chunk
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
    for (int j = tid * 16; j < CHUNK + HALO; j += BLOCK * 16) {
        if (c0 + j + 16 <= a.n) {
            image[1 + (j >> 4)] = *(const uint4*)(a.text + c0 + j);
        } else {
            for (int k = 0; k < 16; k++) s[j + k] = at(a, c0 + j + k);
        }
    }
    if (tid == 0) s[-1] = at(a, c0 - 1);
    __syncthreads();
    int mine = 0;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int o = tid * PER + j;
        if (c0 + o < a.n && starts(s[o - 1], s[o], s[o + 1])) {
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
    const int base = a.w.sum[blockIdx.x];
    for (int k = tid; k < total; k += BLOCK) {
        const int row = base + k - a.skip;
        if (row < 0) continue;                    // a skipped line (the header)
        if (row >= a.max_rows) {
            report(a, K_ROWS, a.max_rows, 0);
            continue;
        }
        parse_row(a, s + first[k], row);
    }
    if (blockIdx.x == 0 && tid == 0) a.w.res[R_LINES] = (unsigned long long)(uint32_t)a.w.sum[a.n_chunks];
}

}  // namespace

extern "C" {

size_t gtf_csv_chunk_bytes(void) { return CHUNK; }

size_t gtf_csv_parse_workspace_bytes(int32_t n_bytes) { return carve(nullptr, n_bytes).total; }

int gtf_csv_parse(const gtf_csv_in* in, gtf_csv_counts* counts, void* workspace, size_t workspace_bytes,
                  gtf_stream_t stream) {
    const char* who = "gtf_csv_parse";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_csv_in", "gtf_csv_in")) return rc;
    if (!counts) return bad("gtf_csv_parse: null counts");
    if (in->n_bytes < 0 || in->skip_lines < 0 || in->max_rows < 0) return bad("gtf_csv_parse: negative sizes");
    if (in->n_bytes > INT32_MAX - 2 * (CHUNK + HALO)) return bad("gtf_csv_parse: a text of 2^31 bytes or more");
    if (in->n_fields < 1 || in->n_fields > MAXF) return bad("gtf_csv_parse: n_fields must be in [1, 64]");
    if (in->n_columns < 0 || in->n_columns > MAXC) return bad("gtf_csv_parse: n_columns must be in [0, 16]");
    const uint8_t d = in->delimiter;
    if ((d >= '0' && d <= '9') || d == '+' || d == '-' || d == '.' || d == 'e' || d == 'E' || d == '"' || d == '\n' ||
        d == '\r' || d == 0)
        return bad("gtf_csv_parse: the delimiter is a character of the number grammar, a quote, a line end or 0");
    if (in->n_bytes > 0 && !in->text) return bad("gtf_csv_parse: null text");
    if ((uintptr_t)in->text % 16) return bad("gtf_csv_parse: text not aligned to 16 bytes");
    Parse a;
    for (int f = 0; f < MAXF; f++) a.req[f] = -1;
    for (int c = 0; c < MAXC; c++) {
        a.type[c] = 0;
        a.out[c] = nullptr;
    }
    for (int c = 0; c < in->n_columns; c++) {
        const gtf_csv_column& q = in->columns[c];
        if (q.field < 0 || q.field >= in->n_fields) {
            snprintf(m, sizeof(m), "gtf_csv_parse: column %d asks for field %d of %d", c, q.field, in->n_fields);
            return bad(m);
        }
        if (q.type != GTF_CSV_INT64 && q.type != GTF_CSV_DOUBLE) return bad("gtf_csv_parse: a column type that is neither GTF_CSV_INT64 nor GTF_CSV_DOUBLE");
        if (a.req[q.field] >= 0) return bad("gtf_csv_parse: a field requested twice");
        if (in->max_rows > 0 && !q.out) return bad("gtf_csv_parse: null output column with max_rows > 0");
        if ((uintptr_t)q.out % 8) return bad("gtf_csv_parse: output column not aligned to 8 bytes");
        a.req[q.field] = (int8_t)c;
        a.type[c] = (uint8_t)q.type;
        a.out[c] = q.out;
    }
    counts->n_rows = 0;
    counts->error = 0;
    counts->first_bad_row = counts->first_bad_field = -1;
    counts->first_bad_error = 0;
    counts->pad_ = 0;
    if (in->n_bytes == 0) return 0;   // no line at all: nothing launched
    if (!workspace || workspace_bytes < gtf_csv_parse_workspace_bytes(in->n_bytes))
        return bad("gtf_csv_parse: workspace smaller than gtf_csv_parse_workspace_bytes");
    a.text = (const uint8_t*)in->text;
    a.n = in->n_bytes; a.skip = in->skip_lines; a.n_fields = in->n_fields; a.max_rows = in->max_rows;
    a.n_chunks = (int32_t)chunks_of(in->n_bytes);
    a.delim = d;
    a.w = carve(workspace, in->n_bytes);
    const Ws& w = a.w;
    const gtf::Cub cub{w.cub, (hipStream_t)stream};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(w.res, 0xff, 8, st)) != hipSuccess) return fail(who, "memset", e);
    if ((e = hipMemsetAsync(w.res + 1, 0, 8 * (R_WORDS - 1), st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_count, dim3(a.n_chunks), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.cnt, w.sum, a.n_chunks + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_parse, dim3(a.n_chunks), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    unsigned long long r[R_WORDS] = {0, 0, 0};
    if ((e = hipMemcpyAsync(r, w.res, sizeof(r), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    const int64_t lines = (int64_t)r[R_LINES], rows = lines > in->skip_lines ? lines - in->skip_lines : 0;
    counts->n_rows = (int32_t)(rows < in->max_rows ? rows : in->max_rows);
    counts->error = (uint32_t)r[R_ERR];
    if (counts->error) {
        counts->first_bad_row = (int32_t)(r[R_KEY] >> 24);
        counts->first_bad_field = (int32_t)((r[R_KEY] >> 8) & 0xffff);
        counts->first_bad_error = 1u << (r[R_KEY] & 0xff);
        snprintf(m, sizeof(m), "gtf_csv_parse: outside the exact domain (error bits 0x%x; first: bit 0x%x at row %d, field %d)",
                 counts->error, counts->first_bad_error, counts->first_bad_row, counts->first_bad_field);
        return bad(m);
    }
    return 0;
}

}  // extern "C"
