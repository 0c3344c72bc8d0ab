"""The last step of BayesHammer's CorrectAllReads restated in Python (no GPU, no engine): the checker of csrc/readprint.hip
and of spades-kmerdata --correct --paired / --correct-stats.

Restated line for line from the reference (paths under assembler/src), on top of tests/readcorrect_restated.py:
  the BH: tags of ReadCorrector::CorrectOneRead     projects/hammer/read_corrector.cpp:210-242
  Read::print with the tag as part of the name      common/io/reads/read.hpp:221-236
  CorrectReadFile's routing                         projects/hammer/hammer_tools.cpp:107-142
  CorrectPairedReadFiles' routing                   projects/hammer/hammer_tools.cpp:144-193

A record is (name, seq, qual): as parsed, qualities with the offset subtracted.
"""
from tests import readcorrect_restated as R

NONE, OK, FAILED, CHANGED = 0, 1, 2, 3
SINGLE_STREAMS = ("good", "bad")
PAIRED_STREAMS = ("cor-left", "cor-right", "unpaired", "bad-left", "bad-right")


def tag_of(rc, seq, qual):
    """(result, new sequence, tag kind, changed) of one TRIMMED read: CorrectReadsBatch's branch on the size
    (hammer_tools.cpp:90-95), then CorrectOneRead (:160-245) with correct_stats_ set"""
    if len(seq) < rc.K:
        return False, seq, NONE, 0
    lleft_pos, lright_pos, solid_len = rc.island(seq, qual)
    res, newseq = rc.correct_one_read(seq, list(qual))
    if solid_len and solid_len != len(seq):  # :202
        corrected = sum(1 for a, b in zip(seq, newseq) if a != b)  # :210-212
        return True, newseq, (CHANGED if corrected else FAILED), corrected  # :214-229
    if solid_len == len(seq):  # :238-242
        return res, newseq, OK, 0
    return res, newseq, NONE, 0


def tag_text(kind, changed):
    """what is appended to the name (:222,227,240)"""
    return ("", " BH:ok", " BH:failed", " BH:changed:" + str(changed))[kind]


def corrected_records(rc, records, trim_quality, tags, offset):
    """[(result, text)] of the records of one file: trimNsAndBadQuality, CorrectReadsBatch, Read::print.  trim_quality
    None: the records are trimmed already (BBK_NO_TRIM) and are taken whole."""
    out = []
    for i, (name, seq, qual) in enumerate(records):
        rc._read = i
        s, q, ltrim, rtrim, initial = R.trim_read(seq, list(qual), trim_quality) if trim_quality is not None else \
            (seq, list(qual), 0, len(seq), len(seq))
        res, newseq, kind, changed = tag_of(rc, s, q)
        shown = name + (tag_text(kind, changed) if tags else "")
        out.append((bool(res), R.read_print(shown, newseq, q, ltrim, rtrim, initial, offset), kind, changed))
    rc._read = None
    return out


def route_single(printed):
    """CorrectReadFile (:135-137): [good text, bad text]"""
    streams = ["", ""]
    for res, text, _, _ in printed:
        streams[0 if res else 1] += text
    return streams


def route_paired(left, right):
    """CorrectPairedReadFiles (:178-186): [cor-left, cor-right, unpaired, bad-left, bad-right]"""
    assert len(left) == len(right)
    streams = ["", "", "", "", ""]
    for (lres, ltext, _, _), (rres, rtext, _, _) in zip(left, right):
        if lres and rres:
            streams[0] += ltext
            streams[1] += rtext
        else:
            streams[2 if lres else 3] += ltext
            streams[2 if rres else 4] += rtext
    return streams
