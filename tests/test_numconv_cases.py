"""tests/numconv_cases.py through the host instantiation of csrc/numconv.hpp, against its exact references, together with the
conditions that keep a pass from coming off the easy paths only (every family present, both tie parities, the exact path reached often
enough, the table-built families really on their branches)."""
import numconv_cases as nc

L = nc.host_lib()


def coverage(texts_by_family, need_idx, modes_need):
    """the conditions on the scan corpus; need_idx: the cases that answered NC_NEED_EXACT in strtod mode without the exact path"""
    fams = {f for f, _ in texts_by_family}
    for f in nc.SCAN_FAMILIES:
        assert f in fams, f
    assert len(need_idx) >= 300
    need_fams = {texts_by_family[i][0] for i in need_idx}
    # both tie parities reach the big-integer comparison, and so do the long tails
    for f in ("midpoint/even", "midpoint/odd", "midpoint/pad%d" % nc.MAX_SIG_DIGITS, "midpoint/pad%d" % (nc.MAX_SIG_DIGITS + 1), "midpoint/pad1200", "sig19_20"):
        assert f in need_fams, f
    # the flag and the grammar's mode do not move a number onto or off the exact path
    assert all(m == need_idx for m in modes_need)


def test_references_agree_with_each_other():
    """the two references of a number's bits -- exact rational arithmetic and glibc -- agree over the corpus, and the restatement of
    strtoimax agrees with libc's: a wrong reference would show here and not as a failure of the code under test"""
    for fam, s in nc.scan_corpus():
        st, bits, used = nc.glibc_strtod(s)
        if st == nc.NC_OK:
            eb = nc.exact_bits(s.split(b"\x00")[0][:used])
            assert eb is None or eb == bits, (fam, s, hex(bits), hex(eb))
    for s in nc.int_texts():
        for base in (10, 16):
            for signed in (1, 0):
                assert nc.ref_intmax(s, base, signed) == nc.libc_intmax(s, base, signed), (s, base, signed)
    # known answers of the rounding itself
    assert nc.exact_bits(nc.midpoint(0).encode()) == 0 and nc.exact_bits((nc.midpoint(0) + "1").encode()) == 1
    assert nc.exact_bits(nc.midpoint(1).encode()) == 2 and nc.exact_bits(nc.midpoint(2).encode()) == 2
    assert nc.exact_bits(nc.midpoint(0x7FEFFFFFFFFFFFFF).encode()) == nc.INF_BITS
    assert nc.exact_bits(str(int(nc.midpoint(0x7FEFFFFFFFFFFFFF)) - 1).encode()) == 0x7FEFFFFFFFFFFFFF
    assert nc.exact_bits(b"-0") == nc.SIGN and nc.exact_bits(b"0x1p-1075") == 0 and nc.exact_bits(b"0x1.8p-1075") == 1
    assert nc.ref_f6(nc.f2b(0.5 / 64 + 0), 400) == b"0.007812" and nc.ref_f6(nc.f2b(3 / 128.0), 400) == b"0.023438"
    assert nc.ref_f6(nc.f2b(-0.0), 400) == b"-0.000000" and nc.ref_f6(nc.SIGN | nc.NAN_BITS, 2) == b"-n"


def test_corpus_is_built_from_the_table():
    pairs = nc.doubt_pairs()
    assert len(pairs) >= 10
    for w, q in pairs:
        hi, lo, refined, doubt, _ = nc.el_product(w, q)
        assert doubt and len(str(w)) == 19
    # the fast path reports them (the exact path does not come back from them: they are kept out of the corpus)
    fam = nc.doubt_family()
    assert len(fam) == 7 * len(pairs) and not set(fam) & {s for _, s in nc.scan_corpus()}
    assert all(r[0] == nc.NC_NEED_EXACT for r in nc.host_scan(L, fam, 0, 0))
    texts = nc.scan_corpus()
    assert sum(1 for f, s in texts if f == "el_refine") >= 50
    for f, s in texts:
        if f == "el_refine":
            w, q = s.decode().split("e")
            assert nc.el_product(int(w), int(q))[2]
    assert sum(len(s) for _, s in texts) < 4 << 20
    assert max(nc.sig_digits(nc.midpoint(b)) for b in nc.midpoint_encodings()) == 768
    for shift in (63, 64):
        assert sum(1 for f, _ in texts if f == "subnormal_shift/%d" % shift) >= 4


def test_scan_double_host():
    corpus = nc.scan_corpus()
    texts = [s for _, s in corpus]
    need = {}
    for mode in nc.MODES:
        ref = [nc.glibc_scan(s, mode) for s in texts]
        assert nc.check_scan(texts, mode, 1, nc.host_scan(L, texts, mode, 1), ref) == []
        need[mode] = nc.check_scan(texts, mode, 0, nc.host_scan(L, texts, mode, 0), ref)
    coverage(corpus, need[0], list(need.values()))
    # NaN payloads are there to be lost: the flag changes some answer
    assert nc.host_scan(L, nc.NANS, 0, 1) != nc.host_scan(L, nc.NANS, nc.NAN_PAYLOAD, 1)


def test_scan_intmax_host():
    texts = nc.int_texts()
    assert len(texts) >= 20000
    for base in (10, 16):
        for signed in (1, 0):
            nc.check_intmax(texts, base, signed, nc.host_intmax(L, texts, base, signed))


def test_fmt_f6_host():
    corpus = nc.f6_corpus()
    assert {f for f, _, _ in corpus} == set(nc.F6_FAMILIES)
    assert {nc.f6_divisor_branch(b) for _, b, _ in corpus} == {None, "k<64", "64<=k<128", "k>=128"}
    vals, caps = [b for _, b, _ in corpus], [c for _, _, c in corpus]
    nc.check_text(nc.OP_FMT_F6, vals, nc.host_text(L, nc.OP_FMT_F6, vals, caps), caps)
    # the ties are ties: seven decimals, the last a 5, and both roundings occur
    ties = [(b, nc.ref_f6(b, 400)) for f, b, _ in corpus if f == "tie"]
    from decimal import Decimal
    assert all(Decimal(nc.b2f(b)).as_tuple().exponent == -7 for b, _ in ties)
    up = sum(1 for b, t in ties if abs(Decimal(t.decode())) > abs(Decimal(nc.b2f(b))))
    assert 0 < up < len(ties)
    assert max(len(nc.ref_f6(b, 400)) for b in vals) == 1 + 309 + 7 and nc.L2M_LABEL_MAX in caps


def test_fmt_json_double_host():
    vals = nc.json_corpus()
    for nan in (0, 1):
        nc.check_text(nc.OP_FMT_JSON, vals, nc.host_text(L, nc.OP_FMT_JSON, vals, p0=nan), p0=nan)


def test_fmt_ld_lu_and_casts_host():
    nc.check_text(nc.OP_FMT_LD, nc.ld_values(), nc.host_text(L, nc.OP_FMT_LD, nc.ld_values()))
    nc.check_text(nc.OP_FMT_LU, nc.lu_values(), nc.host_text(L, nc.OP_FMT_LU, nc.lu_values()))
    i64, u64, dbl = nc.cast_corpus()
    for op, vals in ((nc.OP_I2D, i64), (nc.OP_U2D, u64), (nc.OP_D2I, dbl), (nc.OP_D2U, dbl)):
        nc.check_cast(op, vals, nc.host_cast(L, op, vals))
    # the table of x86-64's answers is what the references say too
    for v, want in nc.CAST_X86_I64:
        assert nc.ref_d2i(v) == (want, 1)
    for v, want in nc.CAST_X86_U64:
        assert nc.ref_d2u(v) == (want, 1)
