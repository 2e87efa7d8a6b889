"""The lanes' count and info words (Lane::totals, tx_info, h_tot, h_info) are addressed by the names of csrc/bmbs_words.h and nowhere
by number: a stage that needs a word claims it in that table.  Reads the sources only (no build, no device)."""
import os
import re

from common import ROOT

CSRC = os.path.join(ROOT, "bitmapperbs_amd", "csrc")
TABLE = "bmbs_words.h"
LITERAL = r"(?<![\w.])\d+\b"            # an integer literal (not the 64 of u64, not a fraction)
FORBIDDEN = {
    "a total addressed by number": r"totals\.as<[^>]*>\(\)\s*(\+\s*\(?\s*\d|\[\s*\d)",
    "a size or offset of totals written as a literal": r"totals\.p\b[^;\n]*?(?<![\w.])[1-9]\d*\b",
    "h_info indexed by number": r"h_info\s*\[\s*\d",
    "h_info offset by number": r"h_info\s*\+\s*\d",
    "h_tot offset by a literal": r"h_tot\s*\+[^;,\n]*?" + LITERAL,
    "a half of tx_info addressed by number": r"tx_info\.as<u32>\(\)\s*\+\s*\d",
}


def sources():
    for f in sorted(os.listdir(CSRC)):
        if f != TABLE and f.endswith((".hip", ".h", ".cpp")):
            yield f, open(os.path.join(CSRC, f)).read()


def test_words_are_addressed_by_name():
    found = []
    for f, text in sources():
        for what, pat in FORBIDDEN.items():
            for m in re.finditer(pat, text):
                found.append("%s:%d: %s: %s" % (f, text.count("\n", 0, m.start()) + 1, what, m.group(0)))
    assert not found, "claim the word in %s and use its name:\n%s" % (TABLE, "\n".join(found))


def test_patterns_catch_the_forms_they_are_for():
    bad = {
        "a total addressed by number": ["c->totals.as<u64>() + 13", "c->totals.as<unsigned long long>() + 13", "c->totals.as<u64>()[2]"],
        "a size or offset of totals written as a literal": ["hipMemsetAsync(c->totals.p, 0, 16 * 8, c->stream)", "hipMemset(c->totals.p, 0, 32 * 8)"],
        "h_info indexed by number": ["if (c->h_info[8])"],
        "h_info offset by number": ["hipMemcpyAsync(c->h_info + 26, x, 8, k, s)"],
        "h_tot offset by a literal": ["c->h_tot + (size_t)slot * 20", "c->h_tot + 16"],
        "a half of tx_info addressed by number": ["c->tx_info.as<u32>() + 8"],
    }
    good = ["hipMemsetAsync(c->totals.p, 0, TOT_CALL_WORDS * sizeof(u64), c->stream)", "c->totals.as<u64>() + t", "CallWords* h = c->h_tot + slot;",
            "c->h_info->stage[TXI_DUP_COUNT]", "c->tx_info.as<u32>() + TXI_STAGE", "c->totals.as<unsigned long long>() + TOT_BIG"]
    for what, lines in bad.items():
        for line in lines:
            assert re.search(FORBIDDEN[what], line), (what, line)
    for line in good:
        for what, pat in FORBIDDEN.items():
            assert not re.search(pat, line), (what, line)


def test_table_is_part_of_the_build_id():
    from bitmapperbs_amd import capi
    assert TABLE in capi.LIB_SRCS
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SHARED\s*:=.*\b%s\b" % re.escape(TABLE), mk, re.M)
