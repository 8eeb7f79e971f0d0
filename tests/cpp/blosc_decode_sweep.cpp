// blosc_decode_sweep — csrc/blosc_decode.hh under the host sanitizers: the
// serial LZ4 block decoder, the frame walker and the unfilter over valid
// blocks and frames, then over seeded mutations of them: bit flips, bytes set
// to 0x00 / 0xFF / 0x0F / 0xF0, truncations, appended bytes, every prefix of
// two blocks of about 600 bytes, and blocks whose offset pair, literal run and
// match run straddle input bytes 255|256 (where the device decoder refills its
// window) — the kinds tests/decode_mutation_cases.py gives the device decoder
// with this code's answers as the expectation.  Every buffer is allocated
// exactly to size, so an access one byte outside a block, a frame, a chunk or
// the scratch is an ASan report.
//
//   make -C acquire-zarr_amd bloscdecodesweep && tests/cpp/bin/blosc_decode_sweep
//
// Host code only: no GPU, no liblz4; the valid inputs come from the serial
// encoder of csrc/lz4_block.hh and a frame writer restated here from
// blosc_frame.cpp's header comment.
#include "blosc_decode.hh"
#include "lz4_block.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <utility>
#include <vector>

namespace {

using Bytes = std::vector<uint8_t>;
using aqz::blosc::Status;

int failures = 0;

#define CHECK(cond, ...)                                                                           \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                            \
            std::printf(__VA_ARGS__);                                                              \
            std::printf("\n");                                                                     \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

// a heap copy of exactly n bytes (n 0: a one-byte allocation nobody may read)
struct Exact
{
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Exact(size_t n_) : p(new uint8_t[n_ ? n_ : 1]), n(n_) {}
    Exact(const uint8_t* s, size_t n_) : Exact(n_)
    {
        if (n_)
            std::memcpy(p.get(), s, n_);
    }
    uint8_t* get() const { return n ? p.get() : nullptr; }
};

Bytes
make_data(std::mt19937& rng, int kind, size_t n)
{
    Bytes v(n);
    for (size_t i = 0; i < n; ++i) {
        switch (kind) {
            case 0: v[i] = uint8_t(rng()); break;
            case 1: v[i] = (rng() % 16) ? 0 : uint8_t(rng()); break;
            case 2: v[i] = uint8_t((i % 37) * 7); break;
            case 3: v[i] = uint8_t(i / 300); break;
            default: v[i] = i >= 64 && (i / 64) % 2 ? v[i - 64] : uint8_t(rng()); break;
        }
    }
    return v;
}

Bytes
encode(const Bytes& src, int accel)
{
    Bytes out(src.size() + src.size() / 255 + 16);
    std::vector<uint32_t> table(aqz::lz4::kTableBytes / 4);
    uint32_t need = 0;
    const uint32_t c = aqz::lz4::encode_block(src.data(), uint32_t(src.size()), out.data(),
                                              uint32_t(out.size()), accel, table.data(), &need);
    out.resize(c);
    return out;
}

void
put32(Bytes& b, size_t at, uint32_t v)
{
    for (int i = 0; i < 4; ++i)
        b[at + i] = uint8_t(v >> (8 * i));
}

// The forward filter, restated from the unfilter's rules (element i byte j ->
// plane j; bit b of byte j of element i -> bit i % 8 of byte i / 8 of row
// j * 8 + b).
void
filter_block(uint32_t filter, uint32_t ts, uint32_t bsize, const uint8_t* src, uint8_t* dst)
{
    const uint32_t kind = aqz::blosc::block_filter(filter, ts, bsize);
    const uint32_t ne = kind == aqz::blosc::kNoFilter ? 0 : bsize / ts;
    std::memset(dst, 0, bsize);
    if (kind == aqz::blosc::kByteShuffle) {
        for (uint32_t i = 0; i < ne; ++i)
            for (uint32_t j = 0; j < ts; ++j)
                dst[size_t(j) * ne + i] = src[size_t(i) * ts + j];
    } else if (kind == aqz::blosc::kBitShuffle) {
        const uint32_t row = ne / 8;
        for (uint32_t i = 0; i < ne; ++i)
            for (uint32_t j = 0; j < ts; ++j)
                for (uint32_t b = 0; b < 8; ++b)
                    dst[size_t(j * 8 + b) * row + i / 8] |=
                      uint8_t(((src[size_t(i) * ts + j] >> b) & 1u) << (i % 8));
    }
    for (size_t o = size_t(ne) * ts; o < bsize; ++o)
        dst[o] = src[o];
}

// A c-blosc style LZ4 frame of `src`: blocks of `bs`, split into typesize
// streams under blosc's rule, splits the encoder cannot shrink stored raw.
Bytes
make_frame(const Bytes& src, uint32_t ts, uint32_t bs, uint32_t filter, int accel)
{
    const uint32_t n = uint32_t(src.size());
    const bool split = ts <= 16 && bs / ts >= 128 && bs % ts == 0;
    const uint32_t nblocks = (n + bs - 1) / bs;
    uint8_t flags = uint8_t(1u << 5);
    flags |= filter == aqz::blosc::kByteShuffle ? 0x1 : filter == aqz::blosc::kBitShuffle ? 0x4 : 0;
    if (!split)
        flags |= 0x10;
    Bytes f(16 + 4 * size_t(nblocks));
    Bytes filt(n);
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t off = b * bs, bsize = n - off < bs ? n - off : bs;
        filter_block(filter, ts, bsize, src.data() + off, filt.data() + off);
        put32(f, 16 + 4 * size_t(b), uint32_t(f.size()));
        const uint32_t nsp = (split && bsize == bs) ? ts : 1;
        const uint32_t neb = bsize / nsp;
        for (uint32_t j = 0; j < nsp; ++j) {
            const Bytes piece(filt.begin() + off + j * neb, filt.begin() + off + (j + 1) * neb);
            Bytes c = encode(piece, accel);
            if (c.size() >= neb)
                c = piece;
            const size_t at = f.size();
            f.resize(at + 4 + c.size());
            put32(f, at, uint32_t(c.size()));
            std::memcpy(f.data() + at + 4, c.data(), c.size());
        }
    }
    f[0] = 2;
    f[1] = 1;
    f[2] = flags;
    f[3] = uint8_t(ts);
    put32(f, 4, n);
    put32(f, 8, bs);
    put32(f, 12, uint32_t(f.size()));
    return f;
}

struct Frame
{
    Bytes bytes, src;
    uint32_t ts;
};

// One sequence of a block written from the format, and where the writer put
// its offset pair and its length-run bytes.
struct Seq
{
    size_t lit;
    uint32_t off, ml;
};

struct Written
{
    Bytes block;
    size_t plain = 0;
    std::vector<size_t> offset_at;
    std::vector<std::vector<size_t>> lit_run, ml_run;
};

void
put_run(Bytes& b, size_t n, std::vector<size_t>* at)
{
    for (n -= 15;; n -= 255) {
        if (at)
            at->push_back(b.size());
        b.push_back(uint8_t(n < 255 ? n : 255));
        if (n < 255)
            break;
    }
}

Written
write_block(std::mt19937& rng, const std::vector<Seq>& seqs, size_t last)
{
    Written w;
    for (const Seq& s : seqs) {
        const size_t m = s.ml - 4;
        w.block.push_back(uint8_t(((s.lit < 15 ? s.lit : 15) << 4) | (m < 15 ? m : 15)));
        w.lit_run.emplace_back();
        w.ml_run.emplace_back();
        if (s.lit >= 15)
            put_run(w.block, s.lit, &w.lit_run.back());
        for (size_t i = 0; i < s.lit; ++i)
            w.block.push_back(uint8_t(rng()));
        w.offset_at.push_back(w.block.size());
        w.block.push_back(uint8_t(s.off));
        w.block.push_back(uint8_t(s.off >> 8));
        if (m >= 15)
            put_run(w.block, m, &w.ml_run.back());
        w.plain += s.lit + s.ml;
    }
    w.block.push_back(uint8_t((last < 15 ? last : 15) << 4));
    if (last >= 15)
        put_run(w.block, last, nullptr);
    for (size_t i = 0; i < last; ++i)
        w.block.push_back(uint8_t(rng()));
    w.plain += last;
    return w;
}

bool
holds(const std::vector<size_t>& v, size_t a, size_t b)
{
    bool fa = false, fb = false;
    for (size_t x : v) {
        fa |= x == a;
        fb |= x == b;
    }
    return fa && fb;
}

// decode a block with both buffers exact; the result is a size within cap or
// a named error
int32_t
decode_block_exact(const Bytes& b, size_t cap)
{
    Exact src(b.data(), b.size()), dst(cap);
    const int32_t r =
      aqz::lz4::decode_block(src.get(), uint32_t(b.size()), dst.get(), uint32_t(cap));
    CHECK(r >= aqz::lz4::kDecEndsInMatch && r <= int32_t(cap), "mutated block of %zu bytes: %d",
          b.size(), r);
    return r;
}

size_t
draw_cap(std::mt19937& rng, size_t n)
{
    switch (rng() % 4) {
        case 0: return n;
        case 1: return n ? n - 1 : 0;
        case 2: return n + 9;
        default: return rng() % (n + 1);
    }
}

const uint8_t kSetValues[4] = { 0x00, 0xFF, 0x0F, 0xF0 };

// decode with every buffer exact; returns the status, fills *out on kOk
Status
decode_exact(const uint8_t* frame, size_t extent, uint32_t ts, uint32_t nbytes, Bytes* out)
{
    Exact f(frame, extent), dst(nbytes), scratch(nbytes);
    aqz::blosc::FrameInfo fi;
    const Status st =
      aqz::blosc::decode_frame_serial(f.get(), extent, ts, nbytes, dst.get(), scratch.get(), &fi);
    if (st == aqz::blosc::kOk && out)
        out->assign(dst.get(), dst.get() + nbytes);
    return st;
}

} // namespace

int
main()
{
    std::mt19937 rng(20261021);
    // ---- blocks ------------------------------------------------------------
    std::vector<Bytes> blocks, plains;
    for (size_t n : { 1u, 5u, 12u, 13u, 14u, 64u, 160u, 300u, 4097u, 20000u, 70000u })
        for (int kind = 0; kind < 5; ++kind) {
            plains.push_back(make_data(rng, kind, n));
            blocks.push_back(encode(plains.back(), 1 + kind * 2));
        }
    size_t n_valid = 0, n_mut = 0, n_refused = 0;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const Bytes& b = blocks[k];
        const size_t n = plains[k].size();
        {
            Exact src(b.data(), b.size()), dst(n);
            const int32_t r = aqz::lz4::decode_block(src.get(), uint32_t(b.size()), dst.get(),
                                                     uint32_t(n));
            CHECK(r == int32_t(n) && std::memcmp(dst.get(), plains[k].data(), n) == 0,
                  "block %zu: %d", k, r);
            ++n_valid;
        }
        for (int m = 0; m < 40; ++m) {
            Bytes mut = b;
            const unsigned what = rng() % 8;
            if (what < 2)
                mut.resize(rng() % mut.size());
            else if (what < 5)
                mut[rng() % mut.size()] ^= uint8_t(1u << (rng() % 8));
            else if (what < 7)
                mut[rng() % mut.size()] = kSetValues[rng() % 4];
            else
                for (unsigned extra = 1 + rng() % 3; extra; --extra)
                    mut.push_back(uint8_t(rng()));
            const int32_t r = decode_block_exact(mut, draw_cap(rng, n));
            ++n_mut;
            n_refused += r < 0;
        }
    }
    // every prefix of two blocks of about 600 bytes: an encoder's, and one of
    // many short sequences written from the format
    {
        std::vector<Seq> seqs;
        size_t plain = 0;
        for (int i = 0; i < 26; ++i) {
            Seq q;
            q.lit = (plain ? 0 : 1) + rng() % 40 + (rng() % 8 ? 0 : 15);
            plain += q.lit;
            q.off = uint32_t(1 + rng() % plain);
            q.ml = rng() % 6 ? uint32_t(4 + rng() % 37) : uint32_t(19 + rng() % 300);
            plain += q.ml;
            seqs.push_back(q);
        }
        const Written w = write_block(rng, seqs, 12);
        const Bytes echo = make_data(rng, 4, 1100);
        const Bytes enc = encode(echo, 1);
        CHECK(decode_block_exact(w.block, w.plain) == int32_t(w.plain), "written block");
        CHECK(w.block.size() > 400 && w.block.size() < 900 && enc.size() > 400 && enc.size() < 900,
              "prefix blocks of %zu and %zu bytes", w.block.size(), enc.size());
        for (const auto& [blk, n] : { std::pair<const Bytes&, size_t>{ w.block, w.plain },
                                      std::pair<const Bytes&, size_t>{ enc, echo.size() } })
            for (size_t cut = 0; cut < blk.size(); ++cut) {
                const int32_t r =
                  decode_block_exact(Bytes(blk.begin(), blk.begin() + cut), draw_cap(rng, n));
                ++n_mut;
                n_refused += r < 0;
            }
    }
    // an offset pair, a literal run and a match run across input bytes 255|256
    {
        size_t n_straddle = 0;
        for (int kind = 0; kind < 3; ++kind)
            for (size_t L = 0; L < 300; ++L) {
                std::vector<Seq> seqs = { { 40, 40, 300 } };
                if (kind == 0) {
                    seqs.push_back({ L, 0x0123, 20 });
                } else if (kind == 1) {
                    seqs.push_back({ L, 7, 8 });
                    seqs.push_back({ 15 + 510 + 9, 300, 8 });
                } else {
                    seqs.push_back({ L, 7, 19 + 510 + 9 });
                }
                const Written w = write_block(rng, seqs, 12);
                const bool hit = kind == 0   ? w.offset_at[1] == 255
                                 : kind == 1 ? holds(w.lit_run[2], 255, 256)
                                             : holds(w.ml_run[1], 255, 256);
                if (!hit)
                    continue;
                ++n_straddle;
                CHECK(decode_block_exact(w.block, w.plain) == int32_t(w.plain), "straddle %d", kind);
                CHECK(decode_block_exact(w.block, w.plain + 9) == int32_t(w.plain), "straddle %d",
                      kind);
                for (size_t at : { size_t(255), size_t(256) })
                    for (unsigned bit = 0; bit < 8; ++bit) {
                        Bytes mut = w.block;
                        mut[at] ^= uint8_t(1u << bit);
                        n_refused += decode_block_exact(mut, draw_cap(rng, w.plain)) < 0;
                        ++n_mut;
                    }
                for (size_t cut : { size_t(255), size_t(256), size_t(257) }) {
                    n_refused += decode_block_exact(Bytes(w.block.begin(), w.block.begin() + cut),
                                                    draw_cap(rng, w.plain)) < 0;
                    ++n_mut;
                }
                break;
            }
        CHECK(n_straddle == 3, "straddling blocks found: %zu", n_straddle);
    }
    // ---- frames ------------------------------------------------------------
    std::vector<Frame> frames;
    struct Shape
    {
        uint32_t ts, n, bs;
    };
    for (const Shape s : { Shape{ 1, 5000, 5000 }, Shape{ 2, 4096, 4096 }, Shape{ 2, 9003, 4096 },
                           Shape{ 3, 3001, 1200 }, Shape{ 4, 8200, 4096 }, Shape{ 8, 8192 + 13, 4096 },
                           Shape{ 16, 1600, 1600 }, Shape{ 16, 5000, 2048 + 16 }, Shape{ 2, 300, 100 } })
        for (uint32_t filter = 0; filter < 3; ++filter)
            for (int kind = 0; kind < 5; ++kind) {
                Frame fr;
                fr.src = make_data(rng, kind, s.n);
                fr.ts = s.ts;
                fr.bytes = make_frame(fr.src, s.ts, s.bs, filter, 1 + kind);
                frames.push_back(std::move(fr));
            }
    size_t f_valid = 0, f_mut = 0, f_refused = 0;
    for (size_t k = 0; k < frames.size(); ++k) {
        const Frame& fr = frames[k];
        const uint32_t n = uint32_t(fr.src.size());
        Bytes out;
        const Status st = decode_exact(fr.bytes.data(), fr.bytes.size(), fr.ts, n, &out);
        CHECK(st == aqz::blosc::kOk && out == fr.src, "frame %zu: status %u", k, unsigned(st));
        ++f_valid;
        for (int m = 0; m < 16; ++m) {
            Bytes mut = fr.bytes;
            const unsigned what = rng() % 12;
            const size_t head = mut.size() < 48 ? mut.size() : 48;
            if (what == 0)
                mut.resize(rng() % mut.size());
            else if (what < 4) // the header, block starts and first sizes steer the walk
                mut[rng() % head] ^= uint8_t(1u << (rng() % 8));
            else if (what < 7)
                mut[rng() % mut.size()] ^= uint8_t(1u << (rng() % 8));
            else if (what < 9)
                mut[rng() % head] = kSetValues[rng() % 4];
            else if (what < 11)
                mut[rng() % mut.size()] = kSetValues[rng() % 4];
            else
                for (unsigned extra = 1 + rng() % 3; extra; --extra)
                    mut.push_back(uint8_t(rng()));
            const Status ms = decode_exact(mut.data(), mut.size(), fr.ts, n, nullptr);
            CHECK(ms <= aqz::blosc::kCorrupt && ms != aqz::blosc::kAbsent, "mutated frame %zu", k);
            ++f_mut;
            f_refused += ms != aqz::blosc::kOk;
        }
    }
    // a memcpy frame, and spans
    {
        Bytes src = make_data(rng, 0, 100), f(116);
        f[0] = 2, f[1] = 1, f[2] = 0x33, f[3] = 2;
        put32(f, 4, 100), put32(f, 8, 100), put32(f, 12, 116);
        std::memcpy(f.data() + 16, src.data(), 100);
        Bytes out;
        CHECK(decode_exact(f.data(), f.size(), 2, 100, &out) == aqz::blosc::kOk && out == src,
              "memcpy frame");
        CHECK(decode_exact(f.data(), 115, 2, 100, nullptr) == aqz::blosc::kBadHeader, "cut");
        const uint64_t words[6] = { 1000, 116, ~0ull, ~0ull, 1090, 20 };
        const auto* table = reinterpret_cast<const uint8_t*>(words);
        aqz::blosc::FrameSpan sp;
        CHECK(aqz::blosc::span_shard(table, 0, 116, 1000, &sp) == aqz::blosc::kOk && sp.offset == 0,
              "span 0");
        CHECK(aqz::blosc::span_shard(table, 1, 116, 1000, &sp) == aqz::blosc::kAbsent, "span 1");
        CHECK(aqz::blosc::span_shard(table, 2, 100, 1000, &sp) == aqz::blosc::kCorrupt, "span 2");
        CHECK(aqz::blosc::span_shard(table, 0, 116, 1001, &sp) == aqz::blosc::kCorrupt, "base");
    }
    std::printf("blocks: %zu valid, %zu mutated (%zu refused); frames: %zu valid, %zu mutated "
                "(%zu refused); %d failures\n",
                n_valid, n_mut, n_refused, f_valid, f_mut, f_refused, failures);
    CHECK(n_mut + f_mut >= 5500 && n_refused > 2000 && f_refused > 800, "too few mutations bite");
    return failures ? 1 : 0;
}
