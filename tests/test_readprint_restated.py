"""CPU: tests/readprint_restated.py pinned on a dozen records whose text is written out by hand from Read::print
(common/io/reads/read.hpp:221-236) and the tag rule of CorrectOneRead (projects/hammer/read_corrector.cpp:214-244).

k = 5 over the ten bases ACGTACCTGA, whose six 5-mers (and their reverse complements) are the good set.  Quality 30 prints
as '?', 10 as '+', 2 as '#' at offset 33; '#' is also Read::print's padding (offset + 2)."""
from tests import readcorrect_restated as R
from tests import readprint_restated as P

K = 5
T = "ACGTACCTGA"
Q = [30] * 10

# (name, sequence, qualities, result, text with tags)
RECORDS = [
    # every start good: solid_len == read_size
    ("ok", T, Q, True, "@ok BH:ok\nACGTACCTGA\n+ok BH:ok\n??????????\n"),
    # the last base wrong at quality 10: the good alternative costs 1, keeping the absent k-mer 3
    ("chg", "ACGTACCTGC", [30] * 9 + [10], True, "@chg BH:changed:1\nACGTACCTGA\n+chg BH:changed:1\n?????????+\n"),
    # the same at quality 30: keeping costs 2, the alternative 5 -- searched, nothing changed
    ("fail", "ACGTACCTGC", Q, True, "@fail BH:failed\nACGTACCTGC\n+fail BH:failed\n??????????\n"),
    # k bases and more, no solid k-mer: CorrectOneRead runs and adds nothing
    ("none", "TTTTTTTT", [30] * 8, False, "@none\nTTTTTTTT\n+none\n????????\n"),
    # fewer than k bases: CorrectOneRead is never called
    ("short", "ACGT", [30] * 4, False, "@short\nACGT\n+short\n????\n"),
    # trimmed to nothing: ltrim_ 0, rtrim_ = initial_size_, two empty lines
    ("gone", "NNNACG", [2] * 6, False, "@gone\n\n+gone\n\n"),
    ("empty", "", [], False, "@empty\n\n+empty\n\n"),
    # left trim only
    ("lt", "NN" + T, [2, 2] + Q, True, "@lt BH:ok\nNNACGTACCTGA\n+lt BH:ok ltrim=2\n##??????????\n"),
    # right trim only
    ("rt", T + "NNN", Q + [2] * 3, True, "@rt BH:ok\nACGTACCTGANNN\n+rt BH:ok rtrim=3\n??????????###\n"),
    # a bad tail of two that the left trim keeps (read.hpp:114): the Ns stay in the read, the right search finds no
    # candidate and fails
    ("kept", "N" + T + "NN", [2] + Q + [2, 2], True, "@kept BH:failed\nNACGTACCTGANN\n+kept BH:failed ltrim=1\n#??????????##\n"),
    # both trims
    ("both", "N" + T + "NNN", [2] + Q + [2] * 3, True,
     "@both BH:ok\nNACGTACCTGANNN\n+both BH:ok ltrim=1 rtrim=3\n#??????????###\n"),
    # the first base wrong at quality 10: corrected by the search on the reverse complement
    ("chg2", "CCGTACCTGA", [10] + [30] * 9, True, "@chg2 BH:changed:1\nACGTACCTGA\n+chg2 BH:changed:1\n+?????????\n"),
]
KINDS = dict(ok=P.OK, chg=P.CHANGED, fail=P.FAILED, none=P.NONE, short=P.NONE, gone=P.NONE, empty=P.NONE, lt=P.OK, rt=P.OK,
             kept=P.FAILED, both=P.OK, chg2=P.CHANGED)


def _corrector():
    index, keys, good = R.make_index(R.kmers_of(T, K))
    return R.ReadCorrector(index, good, K)


def _plain(text):
    for tag in (" BH:ok", " BH:failed", " BH:changed:1"):
        text = text.replace(tag, "")
    return text


def test_records_with_tags():
    rc = _corrector()
    got = P.corrected_records(rc, [r[:3] for r in RECORDS], 4, True, 33)
    for (name, _, _, res, text), (gres, gtext, kind, changed) in zip(RECORDS, got):
        assert (gres, gtext) == (res, text), name
        assert kind == KINDS[name] and changed == (1 if kind == P.CHANGED else 0), name
    assert {k for _, _, k, _ in got} == {P.NONE, P.OK, P.FAILED, P.CHANGED}
    assert rc.stats() == [2, 2, 3, 10 * 7 + 12 + 8]  # kept: the three bases from lright on stay uncorrected


def test_records_without_tags_are_read_print():
    rc = _corrector()
    got = P.corrected_records(rc, [r[:3] for r in RECORDS], 4, False, 33)
    assert [g[1] for g in got] == [_plain(r[4]) for r in RECORDS]
    # and at another offset only the quality line moves
    at64 = P.corrected_records(_corrector(), [RECORDS[7][:3]], 4, False, 64)
    assert at64[0][1] == "@lt\nNNACGTACCTGA\n+lt ltrim=2\nBB^^^^^^^^^^\n"


def test_tag_text():
    assert [P.tag_text(k, 12) for k in range(4)] == ["", " BH:ok", " BH:failed", " BH:changed:12"]


def test_single_routing():
    got = P.corrected_records(_corrector(), [r[:3] for r in RECORDS], 4, True, 33)
    good, bad = P.route_single(got)
    assert good == "".join(r[4] for r in RECORDS if r[3])
    assert bad == "".join(r[4] for r in RECORDS if not r[3])
    assert bad.count("@") == 4


def test_paired_routing():
    by = {r[0]: r for r in RECORDS}
    left = [by[n] for n in ("ok", "none", "chg", "short", "both")]
    right = [by[n] for n in ("fail", "lt", "gone", "empty", "chg2")]
    rc = _corrector()
    streams = P.route_paired(P.corrected_records(rc, [r[:3] for r in left], 4, True, 33),
                             P.corrected_records(rc, [r[:3] for r in right], 4, True, 33))
    text = {n: by[n][4] for n in by}
    assert streams == [text["ok"] + text["both"],      # both mates good: the pair stays a pair
                       text["fail"] + text["chg2"],
                       text["lt"] + text["chg"],      # the good mate of a broken pair, in (pair, left before right) order
                       text["none"] + text["short"],
                       text["gone"] + text["empty"]]
    assert sum(len(s) for s in streams) == sum(len(r[4]) for r in left + right)
