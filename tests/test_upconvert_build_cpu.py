"""The cases of tests/upconvert_build_cases.py hit what they are for, shown without a GPU: the C library converts the number styles to
the values claimed, the out-of-range ones saturate, the tie has equal keys, the shared prefix takes the name sort more than one round."""
import chunk_lib as K
import name_sort_cases as NS
import upconvert_build_cases as UC


def test_styles_convert_to_the_values_claimed():
    for h, want in UC.STYLES.items():
        assert K.decode(h) == want, h
    assert [K.scan_li(t) for t in (b"0x1f", b"017", b"+5", b" 7", b"-3", b"12abc")] == [31, 15, 5, 7, -3, 12]


def test_out_of_range_values_saturate_under_libc():
    assert K.scan_li(b"99999999999999999999") == UC.I64_MAX and K.scan_li(b"-9223372036854775809") == UC.I64_MIN
    for h, want in UC.SATURATING.items():
        assert K.decode(h) == want, h
    table = UC.expected(UC.flat(UC.good_cases()["saturating"]))
    assert table[0][4] == b"big|5|-9223372036854775808" and table[0][1] == UC.I64_MIN
    assert any(t[2] < t[1] for t in table)  # an end that wrapped


def test_the_tie_has_equal_keys_and_keeps_input_order():
    for case, lens in ((UC.TIE_SMALL_FIRST, [10, 100]), (UC.TIE_LARGE_FIRST, [100, 10])):
        recs = UC.flat(case)
        assert len({K.decode(h)[:2] for h, _ in recs}) == 1 and sorted(n for _, n in recs) == [10, 100]
        table = UC.expected(recs)
        assert [t[2] - t[1] for t in table] == lens
    # the probe of two entries looks at the second: found where that is the 100-long interval, the comparator's assert where it is not
    tab = [t[:4] for t in UC.expected(UC.flat(UC.TIE_SMALL_FIRST))]
    assert K.bsearch(tab, b"c", 5, 50) == 1
    tab = [t[:4] for t in UC.expected(UC.flat(UC.TIE_LARGE_FIRST))]
    assert K.bsearch(tab, b"c", 5, 50) == -2


def test_the_shared_prefix_takes_several_rounds():
    recs = UC.flat(UC.good_cases()["shared_prefix"])
    names = UC.names_of(recs)
    assert len(recs) == 600 and len(set(names)) == 300 and all(n.startswith(UC.PREFIX) for n in names)
    order, _, rounds, _ = NS.model(names)
    assert rounds > 1
    assert [names[r] for r in order] == sorted(names)


def test_one_name_cases_cross_a_wave_and_a_block():
    for key, n in (("one_name_65", 65), ("one_name_257", 257)):
        recs = UC.flat(UC.good_cases()[key])
        starts = [K.decode(h)[1] for h, _ in recs]
        assert len(recs) == n and len(set(UC.names_of(recs))) == 1
        assert min(starts) < 0 and max(starts) > 1 << 32 and starts != sorted(starts)
        assert [t[1] for t in UC.expected(recs)] == sorted(starts)


def test_names_prefixes_empty_names_and_nul():
    cases = UC.good_cases()
    assert [t[0] for t in UC.expected(UC.flat(cases["name_prefix"]))] == [b"a", b"a", b"a|b", b"a|b|c"]
    assert [t[:2] for t in UC.expected(UC.flat(cases["empty_name"]))][:3] == [(b"", -4), (b"", 2), (b"", 3)]
    nul = UC.expected(UC.flat(cases["nul"]))
    assert (b"n", 2, 5, 4, b"n|4|2") in nul and not any(b"9" in t[4] for t in nul)


def test_fasta_text_reads_back_and_every_case_is_small():
    for key, case in list(UC.good_cases().items()) + list(UC.bad_cases().items()):
        assert UC.iv_records(UC.texts(case)) == UC.flat(case), key
        assert len(UC.flat(case)) <= 600


def test_failing_headers_fail():
    for h in UC.BAD_HEADERS:
        assert K.decode(h) is None
    for key, case in UC.bad_cases().items():
        assert UC.expected(UC.flat(case)) is None, key
    for key, case in UC.good_cases().items():
        assert UC.expected(UC.flat(case)) is not None, key
