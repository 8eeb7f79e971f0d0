// blosc_decode_sweep — csrc/blosc_decode.hh under the host sanitizers: the
// serial LZ4 block decoder, the frame walker and the unfilter over valid
// blocks and frames, then over seeded single-byte flips and truncations of
// them.  Every buffer is allocated exactly to size, so an access one byte
// outside a block, a frame, a chunk or the scratch is an ASan report.
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
            if (rng() % 4 == 0)
                mut.resize(rng() % mut.size());
            else
                mut[rng() % mut.size()] ^= uint8_t(1u << (rng() % 8));
            const size_t cap = (rng() % 3) ? n : rng() % (n + 1);
            Exact src(mut.data(), mut.size()), dst(cap);
            const int32_t r = aqz::lz4::decode_block(src.get(), uint32_t(mut.size()), dst.get(),
                                                     uint32_t(cap));
            CHECK(r >= aqz::lz4::kDecEndsInMatch && r <= int32_t(cap), "mutated block %zu: %d", k, r);
            ++n_mut;
            n_refused += r < 0;
        }
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
        for (int m = 0; m < 12; ++m) {
            Bytes mut = fr.bytes;
            const unsigned what = rng() % 8;
            if (what == 0)
                mut.resize(rng() % mut.size());
            else if (what < 4) // the header, block starts and first sizes steer the walk
                mut[rng() % (mut.size() < 48 ? mut.size() : 48)] ^= uint8_t(1u << (rng() % 8));
            else
                mut[rng() % mut.size()] ^= uint8_t(1u << (rng() % 8));
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
    CHECK(n_mut + f_mut >= 3000 && n_refused > 200 && f_refused > 200, "too few mutations bite");
    return failures ? 1 : 0;
}
