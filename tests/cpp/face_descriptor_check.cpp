// face_descriptor_check.cpp -- host check of the face descriptor of proton_amd/csrc/face_system.hpp: every field of
// CondFaceLean::packed (seven codes of 6 bits, rows, ncol, the Dirichlet flag) at every value, packed once with all other fields
// zero and once with all other fields all-ones, must come back unchanged with every other field; bits 50-63 stay clear; the record
// is one 16-byte load.  And the parts of a code and of `rows` come back from what fcode_in_A / fcode_in_B / frows_make built.
// Compiled for the host only (tests/test_build_cpu.py); prints the number of packs and exits 0, or the first mismatch and exits 1.
#include <cstdio>

#include "face_system.hpp"

namespace {

struct Fields {
    uint8_t code[7];
    uint32_t rows, ncol;
    bool flag;
};

// field f: 0..6 the codes, 7 rows, 8 ncol, 9 the flag
constexpr uint32_t field_values[10] = {64, 64, 64, 64, 64, 64, 64, 16, 8, 2};

void set_field(Fields &x, int f, uint32_t v)
{
    if (f < 7) x.code[f] = (uint8_t)v;
    else if (f == 7) x.rows = v;
    else if (f == 8) x.ncol = v;
    else x.flag = v != 0;
}

uint32_t get_field(const Fields &x, int f) { return f < 7 ? x.code[f] : f == 7 ? x.rows : f == 8 ? x.ncol : (uint32_t)x.flag; }

Fields unpack(uint64_t p)
{
    Fields x;
    for (uint32_t s = 0; s < 7; ++s) x.code[s] = (uint8_t)pa::lean_code(p, s);
    x.rows = pa::lean_rows(p); x.ncol = pa::lean_ncol(p); x.flag = pa::lean_dirichlet(p);
    return x;
}

}  // namespace

int main()
{
    static_assert(sizeof(pa::CondFaceLean) == 16 && alignof(pa::CondFaceLean) == 16, "one 16-byte load");
    long packs = 0;
    for (int f = 0; f < 10; ++f)
        for (int ones = 0; ones < 2; ++ones)
            for (uint32_t v = 0; v < field_values[f]; ++v) {
                Fields in;
                for (int o = 0; o < 10; ++o) set_field(in, o, ones ? field_values[o] - 1 : 0u);
                set_field(in, f, v);
                const uint64_t p = pa::lean_pack(in.code, in.rows, in.ncol, in.flag);
                ++packs;
                if (p >> 50) { std::printf("field %d value %u others %s: bits 50-63 set (%016llx)\n", f, v, ones ? "ones" : "zero", (unsigned long long)p); return 1; }
                const Fields out = unpack(p);
                for (int o = 0; o < 10; ++o)
                    if (get_field(out, o) != get_field(in, o)) {
                        std::printf("field %d value %u others %s: field %d came back %u, packed %u\n", f, v, ones ? "ones" : "zero", o,
                                    get_field(out, o), get_field(in, o));
                        return 1;
                    }
            }
    // the parts of a code: a column face at local index a of cell A and / or b of cell B
    for (int a = -1; a < 4; ++a)
        for (int b = -1; b < 4; ++b) {
            const uint32_t code = (a >= 0 ? pa::fcode_in_A(a) : 0u) | (b >= 0 ? pa::fcode_in_B(b) : 0u);
            const bool hasA = (code & pa::FCODE_HAS_A) != 0, hasB = (code & pa::FCODE_HAS_B) != 0;
            if (code > 63u || hasA != (a >= 0) || hasB != (b >= 0) || (hasA && pa::fcode_lf_A(code) != (uint32_t)a) ||
                (hasB && pa::fcode_lf_B(code) != (uint32_t)b)) {
                std::printf("code of (A %d, B %d) = %u does not decode\n", a, b, code);
                return 1;
            }
        }
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            const uint32_t rows = pa::frows_make(a, b);
            if (rows > 15u || pa::frows_A(rows) != (uint32_t)a || pa::frows_B(rows) != (uint32_t)b) {
                std::printf("rows of (A %d, B %d) = %u does not decode\n", a, b, rows);
                return 1;
            }
        }
    std::printf("packs %ld ok\n", packs);
    return 0;
}
