"""The host FASTQ reader restated in Python, and the strict four-line index the device builds (csrc/fastqparse.hip,
DESIGN.md 4.3j), with the cases both are held to.

Reader       FastxReader::next_record of host/fastx.hpp, statement by statement: the same getc / getline / strip_cr calls in
             the same order, the same flags.  getline finds its line feed with bytes.find instead of a loop over getc;
             every byte the C++ inspects one at a time is inspected one at a time here.
StrictIndex  record r is lines 4r .. 4r + 3; a record is usable when kseq reads exactly those four lines as name, sequence
             and quality; the verdict is the first record that is not, or whose qualities leave [qvoffset, qvoffset + 93].
"""
import random

FORM, QUALITY = 1, 2  # BBK_FASTQ_FORM, BBK_FASTQ_QUALITY of include/bbk.h
MAX_QUAL = 93


class Reader:
    """FastxReader over `data` from byte `pos`, which must lie between records (what FastxReader::seek leaves)"""

    def __init__(self, data, pos=0):
        self.d, self.p = bytes(data), pos
        self.eof_in = self.eof = self.hit_nl = False
        self.last_char = 0

    def getc(self):
        if self.p >= len(self.d):
            self.eof_in = True
            return -1
        c = self.d[self.p]
        self.p += 1
        return c

    def getline(self, dst):
        """the rest of the current line onto dst (a bytearray or None), without the line feed; False at end of input"""
        self.hit_nl = False
        if self.p >= len(self.d):
            self.eof_in = True
            return False
        e = self.d.find(b"\n", self.p)
        if e < 0:
            if dst is not None:
                dst += self.d[self.p:]
            self.p = len(self.d)
            self.eof_in = True
            return True
        if dst is not None:
            dst += self.d[self.p:e]
        self.p = e + 1
        self.hit_nl = True
        return True

    @staticmethod
    def strip_cr(s, start):
        if len(s) - start > 1 and s[-1] == 0x0D:
            del s[-1]

    def next_record(self):
        """(name, seq, qual) as bytes, or None at the end of the stream"""
        if self.eof:
            return None
        name, out = bytearray(), bytearray()
        if self.last_char == 0:
            while True:
                c = self.getc()
                if c == -1 or c == 0x3E or c == 0x40:
                    break
            if c == -1:
                self.eof = True
                return None
            self.last_char = c
        if not self.getline(name):
            self.eof = True
            return None
        self.strip_cr(name, 0)
        while True:
            c = self.getc()
            if c == -1 or c == 0x3E or c == 0x2B or c == 0x40:
                break
            if c == 0x0A:
                continue
            out.append(c)
            self.getline(out)
            self.strip_cr(out, 0)
        out = bytearray(bytes(out).translate(UPPER))
        self.last_char = c if c in (0x3E, 0x40) else 0
        if c != 0x2B:
            if c == -1:
                self.eof = self.eof_in
            return bytes(name), bytes(out), b""
        self.getline(None)
        if not self.hit_nl:
            self.eof = True
            return None
        q = bytearray()
        while True:
            if not self.getline(q):
                break
            self.strip_cr(q, 0)
            if not len(q) < len(out):
                break
        self.last_char = 0
        if len(q) != len(out):
            self.eof = True
            return None
        return bytes(name), bytes(out), bytes(q)

    def between_records(self):
        return self.last_char == 0


UPPER = bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in range(256))


def records(data, pos=0):
    """every record of the stream from pos"""
    rd, out = Reader(data, pos), []
    while True:
        r = rd.next_record()
        if r is None:
            return out
        out.append(r)


def _strip(data, a, b):
    return b - 1 if b - a > 1 and data[b - 1] == 0x0D else b


class StrictIndex:
    """what bbk_fastq_input_from_host computes for one chunk"""

    def __init__(self, data, final=True, qvoffset=33):
        data = bytes(data)
        self.data = data
        ls, p = [0], 0
        while True:
            e = data.find(b"\n", p)
            if e < 0:
                break
            ls.append(e + 1)
            p = e + 1
        if final and p < len(data):
            ls.append(len(data) + 1)
        self.ls = ls
        self.lines = len(ls) - 1
        self.n = self.lines // 4
        self.fields, self.verdict = [], None
        bases = [0]
        for r in range(self.n):
            l0, l1, l2, l3, l4 = ls[4 * r:4 * r + 5]
            he, se, pe, qe = l1 - 1, l2 - 1, l3 - 1, l4 - 1
            sl, ql = _strip(data, l1, se) - l1, _strip(data, l3, qe) - l3
            form = (he > l0 and data[l0] == 0x40 and (se == l1 or data[l1] not in b"@+>") and pe > l2 and data[l2] == 0x2B
                    and sl == ql)
            name = data[l0 + 1:_strip(data, l0 + 1, he)] if he > l0 else b""
            seq, qual = data[l1:l1 + sl].translate(UPPER), data[l3:l3 + ql]
            self.fields.append((name, seq, qual))
            bases.append(bases[-1] + sl)
            if self.verdict is None:
                if not form:
                    self.verdict = (r, FORM, -1)
                else:
                    bad = [c for c in qual if c < qvoffset or c > qvoffset + MAX_QUAL]
                    if bad:
                        self.verdict = (r, QUALITY, bad[0])
        if self.verdict is None and final and self.lines % 4:
            self.verdict = (self.n, FORM, -1)
        self.usable = self.n if self.verdict is None else self.verdict[0]
        self.bases = bases

    def recs(self, first, n):
        return self.fields[first:first + n]

    def text_end(self, n):
        return 0 if n == 0 else min(self.ls[4 * n], len(self.data))

    def records_within(self, first, max_bases):
        """ReadSource::parse's block rule: a block ends with the record at which its bases reach max_bases"""
        if first >= self.usable:
            return 0
        for r in range(first, self.usable):
            if self.bases[r + 1] - self.bases[first] >= max_bases:
                return r + 1 - first
        return self.usable - first


# ---- cases ---------------------------------------------------------------------------------------------------------------
def fq(name, seq, qual=None, q=b"I", plus=b"+", eol=b"\n"):
    """one four-line record as bytes"""
    name, seq = (x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in (name, seq))
    qual = q * len(seq) if qual is None else (qual.encode("latin-1") if isinstance(qual, str) else bytes(qual))
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


def dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


SEQ_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


def crafted_records(qvoffset=33, seed=5):
    """[(label, record bytes)]: every record is in the strict form"""
    rng = random.Random(seed)
    lo, hi = bytes([qvoffset]), bytes([qvoffset + MAX_QUAL])
    out = [("len%d" % n, fq("len%d" % n, dna(rng, n), q=hi if n % 2 else lo)) for n in SEQ_LENGTHS]
    out += [("lower", fq("lower case", dna(rng, 70, "acgtACGT"))),
            ("nN.", fq("n", "ACGTNnN..acgt" * 5)),
            ("blank name", fq("read 1 with  blanks\tand a tab", dna(rng, 30))),
            ("no name", fq("", dna(rng, 30))),
            ("plus repeats the name", fq("again", dna(rng, 20), plus=b"+again"))]
    for c in (c for c in b"@+>" if qvoffset <= c <= qvoffset + MAX_QUAL):  # (what the offset's range holds of them)
        out.append(("quality begins with %c" % c, fq("q%c" % c, dna(rng, 40), qual=bytes([c]) + hi * 39)))
    out += [("lowest quality", fq("lo", dna(rng, 66), q=lo)), ("highest quality", fq("hi", dna(rng, 66), q=hi)),
            ("crlf", fq("crlf rec", dna(rng, 64), eol=b"\r\n")),
            ("lone cr fields", b"@\r\n\r\n+\n" + hi + b"\n"),
            ("x cr", b"@x\r\nA\r\n+\r\n" + hi + b"\r\n"),
            ("two cr", b"@two\r\r\nAC\r\r\n+\n" + hi * 3 + b"\n")]
    return out


def crafted_text(qvoffset=33):
    return b"".join(r for _, r in crafted_records(qvoffset))


def damaged(kind, rng, qvoffset=33):
    """bytes that stand where a record would: not in the strict form, or with a bad quality byte"""
    s = dna(rng, rng.randrange(2, 120))
    q = bytes([qvoffset + 30]) * len(s)
    h = len(s) // 2
    if kind == "blank line":
        return b"\n" + fq("after a blank line", s)
    if kind == "two-line sequence":
        return b"@two lines\n" + s[:h].encode() + b"\n" + s[h:].encode() + b"\n+\n" + q + b"\n"
    if kind == "missing plus":
        return b"@no plus\n" + s.encode() + b"\n" + q + b"\n"
    if kind == "sequence begins with @":
        return fq("at", "@" + s, q=bytes([qvoffset + 30]))
    if kind == "short quality":
        return b"@short\n" + s.encode() + b"\n+\n" + q[:-1] + b"\n"
    if kind == "long quality":
        return b"@long\n" + s.encode() + b"\n+\n" + q + q[:1] + b"\n"
    if kind == "fasta":
        return b">fasta record\n" + s.encode() + b"\n"
    if kind == "quality below":
        return fq("below", s, qual=q[:h] + bytes([qvoffset - 1]) + q[h + 1:])
    if kind == "quality above":
        return fq("above", s, qual=q[:h] + bytes([qvoffset + MAX_QUAL + 1]) + q[h + 1:])
    raise ValueError(kind)


FORM_DAMAGE = ("blank line", "two-line sequence", "missing plus", "sequence begins with @", "short quality", "long quality",
               "fasta")
QUALITY_DAMAGE = ("quality below", "quality above")
# the damage after which kseq's stream goes on (a quality string of another length ends it, kseq.h:209-212)
FUZZ_DAMAGE = ("blank line", "two-line sequence", "missing plus", "fasta") + QUALITY_DAMAGE


def fuzz_text(seed, n=2000, max_len=300, damage=0.03, qvoffset=33):
    rng = random.Random(seed)
    parts = []
    for i in range(n):
        if rng.random() < damage:
            parts.append(damaged(rng.choice(FUZZ_DAMAGE), rng, qvoffset))
            continue
        m = rng.randrange(max_len + 1)
        qual = bytes(rng.randrange(qvoffset, qvoffset + MAX_QUAL + 1) for _ in range(m))
        parts.append(fq("r%d %s" % (i, "x" * rng.randrange(40)), dna(rng, m, "ACGTNacgt"), qual=qual,
                        eol=b"\r\n" if rng.random() < 0.05 else b"\n"))
    text = b"".join(parts)
    return text[:-1] if seed % 2 else text  # odd seeds: the last line feed is missing


def walk(data, index_of, chunk, qvoffset=33):
    """The records of `data` as a caller of the index gets them: chunks of `chunk` bytes (grown while a chunk holds no
    complete record), the tail carried by text_end; at a verdict the serial reader takes the stream from text_end until it
    is between records again.  index_of(bytes, final) -> an object with n / usable / verdict / text_end / recs(first, n).
    Returns (records, quality verdicts as (record number in the stream, byte))."""
    out, bad, pos, size = [], [], 0, chunk
    while pos < len(data):
        end = min(len(data), pos + size)
        final = end == len(data)
        ix = index_of(data[pos:end], final)
        if ix.usable:
            out += ix.recs(0, ix.usable)
        v = ix.verdict
        if v is None:
            if ix.n == 0 and not final:
                size *= 2
                continue
            pos += ix.text_end(ix.n) if not final else end - pos
            size = chunk
            continue
        if v[1] == QUALITY:
            bad.append((len(out), v[2]))
        rd = Reader(data, pos + ix.text_end(ix.usable))
        while True:
            r = rd.next_record()
            if r is None:
                return out, bad
            out.append(r)
            if rd.between_records():
                break
        pos, size = rd.p, chunk
    return out, bad
