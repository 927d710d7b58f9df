"""Inputs that put the coverage engine of `paffy tile` and `paffy to_bed` on its edges (paffy_amd/csrc/coverage_kernel.h: k_cov_bitmap,
k_cov_walk, k_cov_merge; bed_kernel.h: k_bed_runs, k_bed_lines), and a CPU predictor of what k_cov_bitmap does with a batch. Not a test
module: test_cov_edges_cpu.py proves on the oracle and the predictor that the inputs hit their cases, test_gpu_cov_edges.py runs the same
bytes on the GPU.

Geometry. For a record whose cigar starts at offset cg_off of its batch, round k of the bitmap kernel reads the bytes
[(cg_off & ~15) + k * TEXT, + TEXT): round boundary k lies at cigar byte k * TEXT - (cg_off & 15). A Batch pads the query name of a line
so that cg_off & 15 is what the case asks for; filler ops move a number or a letter to a chosen cigar byte; zero-length ops (`0I0D`) make
a cigar long enough for the four-wave shape without moving a base."""
import os
import re

import oracle_lib as O

# restated from the headers (test_cov_edges_cpu.py::test_constants reads them there)
SHAPES = (64, 256)                       # threads of CovGroup64 / CovGroup256
TEXT = {64: 1024, 256: 4096}             # cigar bytes per round
OPS = {64: 512, 256: 2048}               # op list of a round (TEXT / 2)
WIN = {64: 512, 256: 2048}               # bitmap words of the LDS window
COV_WAVE_BYTES = 9000                    # the longest cigar of the one-wave shape
COV_SLICE = 32768                        # bases per slice of k_cov_walk
BED_PER = 16                             # counters per lane of k_bed_runs
BED_STAGE = 6144                         # bytes of a wave's lines that k_bed_lines stages in LDS
ERR_CHAR, ERR_ASSERT = 4, 19             # PAFFY_ERR_CIGAR_CHAR, PAFFY_ERR_TILE_ASSERT
STRANDS = "+-"
MODES = ("bed", "bed_n", "tile")         # to_bed, to_bed -n, tile


def header_constants(csrc):
    """the same values as the three headers define them: {name: int}"""
    def text(name):
        with open(os.path.join(csrc, name)) as fh:
            return fh.read()

    def value(expr, known):
        expr = re.sub(r"\b(\d+)u\b", r"\1", expr)
        for k, v in known.items():
            expr = re.sub(r"\b%s\b" % k, str(v), expr)
        assert re.fullmatch(r"[\d\s*/+<()-]+", expr), expr
        return int(eval(expr))  # digits and operators only

    cov, host, bed = text("coverage_kernel.h"), text("coverage_host.h"), text("bed_kernel.h")
    out = {}

    def define(src, name):
        out[name] = value(re.search(r"^#define %s[ \t]+(.+?)[ \t]*(?:/\*.*)?$" % name, src, re.M).group(1), out)

    define(cov, "COV_SLICE_SHIFT")
    define(cov, "COV_SLICE")
    define(cov, "COV_TEXT")
    define(cov, "COV_WIN")
    define(host, "COV_WAVE_BYTES")
    define(bed, "BED_PER")
    define(bed, "BED_STAGE")
    for g in SHAPES:
        body = re.search(r"struct CovGroup%d \{(.*?)\n\};" % g, cov, re.S).group(1)
        decl = re.search(r"static constexpr uint32_t (.*?);", body).group(1)
        for name, expr in re.findall(r"(\w+) = ([^,]+)", decl):
            out["%s_%d" % (name, g)] = value(expr, out)
    # the op list: TEXT / 2 entries, in the LDS layout and in the test that sends a round to the serial walk
    assert "G::TEXT / 2 * 8" in cov and "ctot[0] > G::TEXT / 2" in cov
    for g in SHAPES:
        out["OPS_%d" % g] = out["TEXT_%d" % g] // 2
    out["serial_digits"] = int(re.search(r"long_num \|= k >= (\d+)u", cov).group(1))
    return out


# ---- cigar text as the reference reads it (impl/paf.c:86-107: value mod 2^64, then the 56-bit field) ----
_TOKEN = re.compile(rb"(\d*)(\D)|(\d+)$")


def tokens(cg):
    """[(digits, letter or None, index of the letter)] of cigar bytes; digits at the end have no letter"""
    return [(m.group(1), m.group(2), m.start(2)) if m.group(2) is not None else (m.group(3), None, len(cg)) for m in _TOKEN.finditer(cg)]


def l56(digits):
    v = (int(digits or b"0") % (1 << 64)) & ((1 << 56) - 1)
    return v - (1 << 56) if v >> 55 else v


_SPANS = {}


def spans(cg):
    """(query bases, target bases, aligned bases) of a cigar without a bad letter"""
    if cg not in _SPANS:
        _SPANS[cg] = _spans(cg.encode() if isinstance(cg, str) else cg)
    return _SPANS[cg]


def _spans(cg):
    q = t = a = 0
    for d, c, _ in tokens(cg):
        assert c is not None and c in b"MIDX=", (d, c)
        n = l56(d)
        if c != b"D":
            q += n
        if c != b"I":
            t += n
        if c in b"M=X":
            a += n
    return q, t, a


_FILL = ("13M", "2I", "11M", "3D", "1M", "10M", "100M")
_NULL = ("00I", "0D", "00D", "0I", "0I", "00D", "000I")  # ops of no length: text that moves no base


def filler(nbytes, phase=0, toks=_FILL):
    """ops whose text is exactly nbytes long (0, or 2 and more): 13M 2I 11M 3D ..., the rest in one M op"""
    assert nbytes == 0 or nbytes >= 2, nbytes
    out, rem, i = [], nbytes, phase
    while rem > 4:
        out.append(toks[i & 3])
        rem -= len(out[-1])
        i += 1
    if rem:
        out.append(toks[2 + rem])
    return "".join(out)


def to_shape(cg, g, pad="0I0D"):
    """the cigar as the shape g takes it: for the four-wave shape zero-length ops behind it until it is longer than COV_WAVE_BYTES"""
    if g == 64:
        assert len(cg) <= COV_WAVE_BYTES, len(cg)
        return cg
    if len(cg) <= COV_WAVE_BYTES:
        cg += pad * ((COV_WAVE_BYTES - len(cg)) // len(pad) + 1)
    assert len(cg) > COV_WAVE_BYTES
    return cg


def line(cg, strand="+", qname="q", tname="t", qs=0, ts=0, qtail=3, ttail=5, qe=None, te=None, qlen=None, tlen=None, front="", back="", score=None, spans_of=None):
    """a PAF line whose coordinates fit its cigar unless qe / te / qlen / tlen say otherwise; spans_of: the cigar the coordinates are taken
    from when cg itself cannot be read (a bad letter)"""
    q, t, a = spans(spans_of if spans_of is not None else cg)
    qe = qs + q if qe is None else qe
    te = ts + t if te is None else te
    qlen = qe + qtail if qlen is None else qlen
    tlen = te + ttail if tlen is None else tlen
    tags = ([front] if front else []) + (["AS:i:%d" % score] if score is not None else []) + (["cg:Z:" + cg] if cg is not None else []) + ([back] if back else [])
    return "\t".join([qname, str(qlen), str(qs), str(qe), strand, tname, str(tlen), str(ts), str(te), str(a), str(max(q, t)), "60"] + tags) + "\n"


class Batch:
    """lines back to back; add() pads the query name so that the cigar's first byte lies at offset `off` (mod 16) of the batch"""

    def __init__(self, name, error_free=True):
        self.name, self.error_free = name, error_free
        self.lines, self.expect, self.size, self._data = [], [], 0, None

    def add(self, cg, off=None, expect=None, raw=None, **kw):
        i = len(self.lines)
        kw.setdefault("qname", "q%d" % i)
        kw.setdefault("tname", "t%d" % i)
        text = raw if raw is not None else line(cg, **kw)
        if off is not None:
            assert raw is None
            at = self.size + text.index("cg:Z:") + 5
            kw["qname"] += "x" * ((off - at) % 16)
            text = line(cg, **kw)
            assert (self.size + text.index("cg:Z:") + 5) % 16 == off
        self.lines.append(text)
        self.expect.append(dict(expect or {}))
        self.size += len(text)
        return i

    @property
    def data(self):
        if self._data is None or len(self._data) != self.size:
            self._data = "".join(self.lines).encode()
        return self._data


# ---- the predictor: what k_cov_bitmap does with every line of a batch ----
def _fields(ln):
    f = ln.rstrip(b"\n").split(b"\t")
    cg_at = None
    at = 0
    for k, x in enumerate(f):
        if k >= 12 and x.startswith(b"cg:Z:"):
            cg_at = at + 5
        at += len(x) + 1
    return f, cg_at


def predict(data, sides=1):
    """Per line of the batch a dict: cg_off, cg_len, shape, rounds, letters (per round), boundary (cigar byte of every round's start),
    serial (None or (why, round): "digits" -- a number of eight or more digits, "letters" -- more letters than the op list), straddles
    [(round, digits in front of the boundary, digits)], first_letter / last_letter (rounds that begin / end with a letter), and per walked side
    (0 query; with sides == 2 also 1 / 2: the target of a + / - record) `lds`: for every round up to the serial one True (window), False
    (straight into HBM) or None (nothing to set), with `words` the size of its range."""
    out, base = [], 0
    for ln in data.splitlines(keepends=True):
        f, cg_at = _fields(ln)
        p = dict(has_cg=cg_at is not None)
        out.append(p)
        if cg_at is None:
            base += len(ln)
            continue
        cg = f[[k for k, x in enumerate(f) if k >= 12 and x.startswith(b"cg:Z:")][0]][5:]
        cg_off, n = base + cg_at, len(cg)
        base += len(ln)
        g = 64 if n <= COV_WAVE_BYTES else 256
        T = TEXT[g]
        lead = cg_off & 15
        rounds = (lead + n + T - 1) // T if n else 0
        toks = tokens(cg)
        rnd = lambda i: (i + lead) // T  # noqa: E731 -- the round of cigar byte i
        letters = [0] * rounds
        by_round = [[] for _ in range(rounds)]
        for d, c, i in toks:
            if c is not None:
                letters[rnd(i)] += 1
                by_round[rnd(i)].append((d, c))
        serial = None
        for k in range(rounds):
            if letters[k] > OPS[g]:
                serial = ("letters", k)
            elif any(len(d) >= 8 for d, _ in by_round[k]):
                serial = ("digits", k)
            if serial:
                break
        bounds = [k * T - lead for k in range(rounds)]
        straddles = []
        for d, c, i in toks:
            s = i - len(d)
            for k in range(1, rounds):
                if s < bounds[k] < i:
                    straddles.append((k, bounds[k] - s, len(d)))
        is_letter = lambda i: 0 <= i < n and not 48 <= cg[i] <= 57  # noqa: E731
        p.update(cg_off=cg_off, cg_len=n, lead=lead, shape=g, rounds=rounds, letters=letters, boundary=bounds, serial=serial, straddles=straddles,
                 first_letter=[k for k in range(1, rounds) if is_letter(bounds[k])], last_letter=[k for k in range(rounds) if is_letter(bounds[k] + T - 1)],
                 sides={})
        plus = f[4] == b"+"
        for side in ([0] + ([1 if plus else 2] if sides == 2 else [])):
            start, end, length = (int(f[2]), int(f[3]), int(f[1])) if side == 0 else (int(f[7]), int(f[8]), int(f[6]))
            skip = b"D" if side == 0 else b"I"
            lo = min(max(start, 0), max(length, 0))
            hi = max(min(end, max(length, 0)), lo)
            cur, lds, words = start, [], []
            for k in range(rounds if serial is None else serial[1]):
                t0 = sum(int(d or b"0") for d, c in by_round[k] if (c if c in b"MIDX=" else b"D") != skip)
                t1 = sum(int(d or b"0") for d, c in by_round[k] if c in b"M=X")
                r_lo, r_hi = (start + end - (cur + t0), start + end - cur) if side == 2 else (cur, cur + t0)
                c_lo, c_hi = max(r_lo, lo), min(r_hi, hi)
                if c_hi > c_lo and t1 > 0:
                    w = ((c_hi - 1) >> 5) - (c_lo >> 5) + 1
                    words.append(w)
                    lds.append(w <= WIN[g])
                else:
                    words.append(0)
                    lds.append(None)
                cur += t0
            p["sides"][side] = dict(lds=lds, words=words)
    return out


# ---- running a batch ----
_WANT = {}


def oracle(mode, data, **kw):
    """(error code, error record, output) of the oracle; mode: one of MODES"""
    key = (mode, data, tuple(sorted(kw.items())))
    if key not in _WANT:
        if mode == "tile":
            out, err = O.tile(data)
        else:
            out, err = O.to_bed(data, include_inverted=(mode == "bed_n"), **kw)
        _WANT[key] = (err.code, err.record, out)
    return _WANT[key]


def gpu(eng, mode, data, batch_bytes=None, **kw):
    if mode == "tile":
        got, info = eng.tile(data, raise_on_error=False, batch_bytes=batch_bytes)
    else:
        got, info = eng.to_bed(data, raise_on_error=False, include_inverted=(mode == "bed_n"), batch_bytes=batch_bytes, **kw)
    return info.error.code, info.error.record, got


def check(eng, data, modes=MODES, batch_bytes=None, **kw):
    """byte equality with the oracle, and the same error code and record"""
    for mode in modes:
        wcode, wrec, want = oracle(mode, data, **(kw if mode != "tile" else {}))
        code, rec, got = gpu(eng, mode, data, batch_bytes, **(kw if mode != "tile" else {}))
        assert code == wcode and (wcode == 0 or rec == wrec), (mode, kw, code, wcode, rec, wrec)
        assert len(got) == len(want) and got == want, (mode, kw, len(got), len(want), first_difference(got, want))


def first_difference(a, b):
    la, lb = a.splitlines(), b.splitlines()
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return i, x[:120], y[:120]
    return min(len(la), len(lb)), None, None


# ---- group 1: alignment ----
def alignment_batches():
    """the cigar's first byte at each offset of a 16-byte chunk, in both shapes; cigars of 1, 2, 15, 16, 17 bytes at each offset (by their
    length one-wave entries); a tag behind the cigar, the next line right behind it, the next line's name beginning with digits"""
    long_ = Batch("align_first_byte")
    for g in SHAPES:
        for off in range(16):
            for s in STRANDS:
                long_.add(to_shape("21M" + filler(300 + off, off), g), off, dict(shape=g, lead=off), strand=s, qs=off, ts=3 * off)
    tiny = Batch("align_tiny")
    texts = {1: "M", 2: "7M", 15: "10M2I11M3D1234M", 16: "10M2I11M3D12M34M", 17: "10M2I11M3D1M1234M"}
    i = 0
    for off in range(16):
        for n, cg in texts.items():
            assert len(cg) == n
            # digits at the start of the next line's name: read as a number if the cigar's end is mistaken
            tiny.add(cg, off, dict(shape=64, lead=off, cg_len=n), strand=STRANDS[i & 1], qs=off + 1, ts=2, back="zz:i:5" if i % 3 == 0 else "",
                     qname=("77q%d" if i % 2 else "q%d") % i)
            i += 1
    ends = Batch("align_last_byte")
    for g in SHAPES:
        for want_end in (15, 0, 1):  # the last byte is the last / first byte of a chunk, or the first but one
            for s in STRANDS:
                base = to_shape("9M" + filler(200), g)
                extra = (want_end - (3 + len(base) - 1)) % 16
                cg = "1" + base if extra == 1 else base + (filler(extra) if extra else "")
                assert (3 + len(cg) - 1) % 16 == want_end
                ends.add(cg, 3, dict(shape=g, last_at=want_end), strand=s, qname="55q%d" % len(ends.lines))
    return [long_, tiny, ends]


def threshold_batch():
    """cigars of exactly COV_WAVE_BYTES and one byte more: the last entry of the one-wave shape and the first of the other"""
    b = Batch("threshold")
    for n in (COV_WAVE_BYTES, COV_WAVE_BYTES + 1):
        for s in STRANDS:
            for lead in (0, 11):
                b.add(filler(n, lead), lead, dict(cg_len=n, shape=64 if n == COV_WAVE_BYTES else 256), strand=s, qs=9)
    return b


# ---- group 2: numbers across a round boundary ----
def straddle_number(n, j):
    """n digits, the first j in front of the boundary with a digit that counts among them: the value changes when they are lost"""
    return "0" * (j - 1) + "1" + "0" * (n - j - 1) + "2"


def straddle_cigar(g, at, lead, n, j, letter="M"):
    """a number of n digits of which j lie in front of byte `at` of the kernel's text (at = k * TEXT: round boundary k), the cigar
    starting `lead` bytes into its 16-byte chunk"""
    front = at - lead - j
    return to_shape(filler(front) + straddle_number(n, j) + letter + filler(40, 1), g, pad=filler(10))


def without_front_digits(cg, at, lead, j):
    front = at - lead - j
    return cg[:front] + cg[front + j:]


def straddle_batches():
    out = []
    for g in SHAPES:
        for k in (1, 2):
            b = Batch("straddle_%d_round_%d" % (g, k))
            for n in range(2, 8):
                for j in range(1, n):
                    for s in STRANDS:
                        lead = (5 * n + j) % 16
                        cg = straddle_cigar(g, k * TEXT[g], lead, n, j)
                        b.add(cg, lead, dict(shape=g, straddle=(k, j, n), at=k * TEXT[g], serial=None), strand=s, qs=17, ts=29)
            out.append(b)
        b = Batch("straddle_%d_lane" % g)  # a 16-byte lane boundary inside round 0 (lane 5 | 6) and inside round 1
        for at in (96, TEXT[g] + 160):
            for n in range(2, 8):
                for j in range(1, n):
                    lead = (3 * n + j) % 16
                    b.add(straddle_cigar(g, at, lead, n, j), lead, dict(shape=g, lane=(at, j, n), at=at, serial=None), strand=STRANDS[(n + j) & 1], qs=5, ts=31)
        out.append(b)
        b = Batch("letter_on_round_edge_%d" % g)
        for k in (1, 2):
            for s in STRANDS:
                for lead in (0, 7):
                    at = k * TEXT[g] - lead  # cigar byte of the boundary
                    b.add(to_shape(filler(at - 2) + "17M" + filler(30, 1), g, pad=filler(10)), lead, dict(shape=g, first_letter=k), strand=s)  # M is the round's first byte
                    b.add(to_shape(filler(at - 3) + "17M" + "5I" + filler(30, 1), g, pad=filler(10)), lead, dict(shape=g, last_letter=k - 1), strand=s)
                    b.add(to_shape(filler(at) + "M23M" + filler(30, 1), g, pad=filler(10)), lead, dict(shape=g, first_letter=k, last_letter=k - 1), strand=s)  # a digitless op first
        out.append(b)
    return out


# ---- group 3: the serial path ----
SERIAL_NUMBERS = {"eight": "00000100", "nine": "000000100", "twenty": "00000000000000000100", "two_pow_56_plus_10": str((1 << 56) + 10)}


def serial_batches():
    out = []
    for g in SHAPES:
        b = Batch("serial_digits_%d" % g)
        for name, num in sorted(SERIAL_NUMBERS.items()):
            for k in (0, 2):
                for s in STRANDS:
                    lead = (len(num) + k) % 16
                    front = filler(k * TEXT[g] + 100 - lead) if k else "5M2I"
                    b.add(to_shape(front + num + "M" + filler(60, 1), g, pad=filler(10)), lead, dict(shape=g, serial=("digits", k)), strand=s, qs=33, ts=1)
        out.append(b)
        b = Batch("serial_letters_%d" % g)
        full, dense = "1M1I" * (TEXT[g] // 4), "1M1I" * (TEXT[g] // 4 - 1) + "1MMI"
        for k in (0, 2):
            for s in STRANDS:
                lead = 0 if k == 0 else 6
                front = filler(k * TEXT[g] - lead) if k else ""
                b.add(to_shape(front + full + filler(50), g, pad=filler(10)), lead, dict(shape=g, serial=None, letters=(k, OPS[g])), strand=s, qs=2)
                b.add(to_shape(front + dense + filler(50), g, pad=filler(10)), lead, dict(shape=g, serial=("letters", k), letters=(k, OPS[g] + 1)), strand=s, qs=2)
        out.append(b)
    return out


def negative_wrap_batches():
    """a length with bit 55 set is negative in the 56-bit field: the walk steps back, the reference's position assert fires"""
    out = []
    for g in SHAPES:
        for k in (0, 2):
            b = Batch("serial_negative_%d_round_%d" % (g, k), error_free=False)
            b.add("10M", qname="ok", tname="okt", qlen=40, tlen=40)
            front = filler(k * TEXT[g] + 100) if k else "5M"
            q, t, _ = spans(front)
            cg = to_shape(front + str((1 << 55) + (1 << 56) * 3) + "M" + "7M", g, pad=filler(10))
            raw = line(cg, qe=50 + q + 7, te=60 + t + 7, qs=50, ts=60, qlen=200000, tlen=200000, spans_of="1M", qname="neg", tname="negt")
            b.add(None, raw=raw, expect=dict(shape=g, serial=("digits", k), err={m: ERR_ASSERT for m in MODES}))
            b.add("10M", qname="ok", tname="okt", qs=20, ts=20, qlen=40, tlen=40)
            out.append(b)
    return out


# ---- group 4: degenerate ops ----
def degenerate_batch():
    b = Batch("degenerate")
    for g in SHAPES:
        for s in STRANDS:
            b.add(to_shape("0M5M0I3M0D0M2I0D4M", g), 9, dict(shape=g), strand=s)
            b.add(to_shape("0M", g), 1, dict(shape=g), strand=s)
            b.add(to_shape("5=3X2I4=1D7X", g), 12, dict(shape=g), strand=s, qs=30)
            # a round of nothing but I and D ops between two rounds with bits
            lead = 4
            mid = "2I3D" * ((TEXT[g]) // 4)
            b.add(to_shape(filler(TEXT[g] - lead) + mid + "40M" + filler(20), g, pad=filler(10)), lead, dict(shape=g, idle_round=1), strand=s, qs=31)
    return b


# ---- group 5: errors ----
def error_batches():
    """an error-free line in front and behind: the failing record is record 1"""
    out = []

    def case(name, cg, expect_err, g, lead=None, spans_of=None, **kw):
        b = Batch("err_%s_%d" % (name, g), error_free=False)
        b.add("10M", qname="ok", tname="okt", qlen=40, tlen=40)
        kw.setdefault("qname", "bad")
        kw.setdefault("tname", "badt")
        b.add(cg, lead, dict(shape=g, err=expect_err), spans_of=spans_of, **kw)
        b.add("10M", qname="ok", tname="okt", qs=20, ts=20, qlen=40, tlen=40)
        out.append(b)
        return b

    every = lambda c: {m: c for m in MODES}  # noqa: E731
    for g in SHAPES:
        T = TEXT[g]
        for s in STRANDS:
            good = to_shape(filler(T - 5 - 2) + "17M" + filler(30, 1), g, pad=filler(10))
            bad = good[:T - 5] + "Q" + good[T - 5 + 1:]
            case("bad_letter_first_of_round_" + s, bad, every(ERR_CHAR), g, 5, spans_of=good, strand=s)
            good = to_shape(filler(T - 5 - 3) + "17M" + filler(30, 1), g, pad=filler(10))
            bad = good[:T - 5 - 1] + "S" + good[T - 5:]
            case("bad_letter_last_of_round_" + s, bad, every(ERR_CHAR), g, 5, spans_of=good, strand=s)
        for end_at in range(16):  # the cigar ends in digits whose last lies at every offset of a chunk
            body = to_shape("7M" + filler(60), g)
            extra = (end_at - (2 + len(body) + 1)) % 16
            cg = body + "1" * (extra + 2)  # at least two digits
            assert (2 + len(cg) - 1) % 16 == end_at
            case("trailing_digits_%d" % end_at, cg, every(ERR_CHAR), g, 2, spans_of=body)
        lead = 3
        body = filler((2 if g == 64 else 3) * T - lead - 2)
        cg = body + "12"
        assert (lead + len(cg)) % T == 0 and (g == 64) == (len(cg) <= COV_WAVE_BYTES)
        case("trailing_digits_on_round_boundary", cg, every(ERR_CHAR), g, lead, spans_of=body)
        # the walk is already past query_end when the bad letter comes: the character error wins (cigar_parse runs first)
        good = to_shape("30M" + filler(2 * T) + "5M", g, pad=filler(10))
        bad = good[:-2] + "5Q"
        case("bad_letter_after_overrun", bad, every(ERR_CHAR), g, 11, spans_of=good, qe=20, qlen=9000000)
        for s in STRANDS:
            cg = to_shape("30M" + filler(T + 40) + "5M", g, pad=filler(10))
            q, t, _ = spans(cg)
            for d in (-1, 1):
                tag = "short" if d < 0 else "past"
                case("query_walk_one_%s_%s" % (tag, s), cg, every(ERR_ASSERT), g, 8, strand=s, qs=40, qe=40 + q + d, qlen=40 + q + 9)
                case("target_walk_one_%s_%s" % (tag, s), cg, dict(bed=0, bed_n=ERR_ASSERT, tile=0), g, 8, strand=s, ts=40, te=40 + t + d, tlen=40 + t + 9)
    return out


# ---- group 6: window or HBM ----
def round_of(nbytes, bases, last="9M"):
    """one round's text: exactly nbytes, `bases` query bases, an M op first and last so that neighbouring rounds meet inside a word"""
    for digits in range(1, 9):
        mid = filler(nbytes - digits - 1 - len(last), 1, _NULL)
        big = bases - spans(mid)[0] - spans(last)[0]
        if big > 0 and len(str(big)) == digits:
            return "%dM" % big + mid + last
    raise AssertionError((nbytes, bases))


def window_batches():
    out = []
    for g in SHAPES:
        T, W = TEXT[g], WIN[g]
        b = Batch("window_exact_%d" % g)
        for s in STRANDS:
            for words in (W, W + 1):
                # round 0 covers exactly `words` words from a word boundary on; round 1 goes on in the window
                lead = 4
                cg = round_of(T - lead, 32 * (words - 1) + 1) + round_of(T, 500) + filler(30)
                b.add(to_shape(cg, g), lead, dict(shape=g, lds0=(words <= W), words0=words), strand=s, qs=64, ts=7)
        out.append(b)
        b = Batch("window_alternating_%d" % g)
        for s in STRANDS:
            lead = 9
            sizes = [32 * W + 333, 777, 32 * (W + 3) + 5, 45, 64 * W + 1]
            cg = round_of(T - lead, sizes[0]) + "".join(round_of(T, x) for x in sizes[1:]) + "3M"
            b.add(to_shape(cg, g), lead, dict(shape=g, lds=[False, True, False, True, False]), strand=s, qs=7, ts=13)
        out.append(b)
    b = Batch("window_one_op_millions")
    for s in STRANDS:
        b.add("5000000M", 6, dict(shape=64, lds=[False]), strand=s, qs=12345, ts=77, qname="big_q" + s, tname="big_t" + s)
        b.add(to_shape("6000001M" + filler(100), 256, pad=filler(10)), 6, dict(shape=256), strand=s, qs=3, ts=2, qname="big4_q" + s, tname="big4_t" + s)
    out.append(b)
    return out


# ---- group 7: word, slice and sequence boundaries ----
EDGES = (31, 32, 33, COV_SLICE - 1, COV_SLICE, COV_SLICE + 1)
SEQ_LENGTHS = (1, 7, 8, 9, 16, 17, 32767, 32768, 32769, 65537)


def boundary_records():
    """[(name, keyword arguments of line(), cigar)]: every record on sequences of its own"""
    recs = []
    for a in EDGES:
        for b in EDGES:
            if a < b:
                recs.append(("op_%d_%d" % (a, b), dict(qs=a, ts=a, qtail=40, ttail=40), "%dM" % (b - a)))
    for e in EDGES:  # an op boundary (not the record's) on the edge: M | I | M and M | D | M
        recs.append(("inner_%d" % e, dict(qs=3, ts=3), "%dM2I%dM3D4M" % (e - 3, 5)))
    recs.append(("last_base_of_slice_to_first_of_next", dict(qs=COV_SLICE - 1, ts=COV_SLICE - 1), "2M"))
    recs.append(("second_slice_boundary", dict(qs=2 * COV_SLICE - 1, ts=2 * COV_SLICE - 1), "2M"))
    for n in SEQ_LENGTHS:
        recs.append(("whole_sequence_%d" % n, dict(qs=0, ts=0, qtail=0, ttail=0), "%dM" % n))
        if n > 1:
            recs.append(("last_base_of_%d" % n, dict(qs=n - 1, ts=n - 1, qtail=0, ttail=0), "1M"))
            recs.append(("all_but_last_of_%d" % n, dict(qs=0, ts=0, qtail=1, ttail=1), "%dM" % (n - 1)))
    recs.append(("start_equals_end_query", dict(qs=40, ts=10), "4D"))
    recs.append(("start_equals_end_target", dict(qs=40, ts=10), "4I"))
    recs.append(("start_equals_end_both", dict(qs=40, ts=10), "0M"))
    return recs


def boundary_batch(g, moved=False):
    """moved: every record one base further on sequences of the same length -- one base back where it ends with its sequence, one base
    shorter where it covers it (the CPU test's sharpness check)"""
    b = Batch("boundaries_%d" % g)
    for i, (name, kw, cg) in enumerate(boundary_records()):
        q, t, _ = spans(cg)
        kw = dict(kw, qlen=kw["qs"] + q + kw.get("qtail", 3), tlen=kw["ts"] + t + kw.get("ttail", 5))
        if moved:
            step = 1 if kw.get("qtail", 3) > 0 else -1
            if kw["qs"] + step < 0:
                cg = "%dM" % (q - 1)
            else:
                kw["qs"] += step
                kw["ts"] += step
        b.add(to_shape(cg, g), None, dict(shape=g, name=name), strand=STRANDS[i & 1], qname="q_" + name, tname="t_" + name, **kw)
    return b


def bed_by_name(out):
    """{sequence name: its lines} of a to_bed output"""
    d = {}
    for ln in out.splitlines():
        d.setdefault(ln.split(b" ")[0], []).append(ln)
    return d


# ---- group 9: k_bed_runs ----
def runs_batch():
    """sequences laid back to back (each at a multiple of 8 counters, 8 or more of padding behind it): ends at every position of a lane's
    sixteen counters, lengths that are multiples of 16 and of 4 096, neighbours whose last and first counters are equal, one-base sequences"""
    b = Batch("bed_runs")
    k = 0
    for n in list(range(1, 50)) + [64, 4096, 8192, 4096 + 16, 12288]:
        for cover in ("none", "all", "first", "last", "inner"):
            if cover == "inner" and n < 3:
                continue
            qs, span = {"none": (0, 0), "all": (0, n), "first": (0, max(1, n // 3)), "last": (n - max(1, n // 3), max(1, n // 3)), "inner": (1, n - 2)}[cover]
            b.add("%dM" % span if span else "3D", None, dict(), qs=qs, qlen=n, qname="r%d_%s" % (n, cover), tname="T", ts=k % 50, tlen=20000, strand=STRANDS[k & 1])
            k += 1
    for i in range(300):  # one-base sequences: covered, covered twice, not at all
        if i % 3 == 2:
            b.add("2D", None, dict(), qs=0, qlen=1, qname="one%d" % i, tname="T", ts=0, tlen=20000)
        else:
            for _ in range(1 + i % 3):
                b.add("1M", None, dict(), qs=0, qlen=1, qname="one%d" % i, tname="T", ts=i % 90, tlen=20000)
    return b


# ---- group 10: k_bed_lines ----
LINE_NAMES = (1, 84, 85, 86, 87, 88, 89, 90, 91, 92, 95, 97, 300)  # 64 lines of name + 7 to name + 9 bytes: BED_STAGE is 64 * 96


def wave_spans(batch, out):
    """bytes of every wave's 64 lines in k_bed_lines: the runs of all sequences in order, one more per sequence for the padding behind it"""
    by, sizes, seen = bed_by_name(out), [], set()
    for ln in batch.lines:
        name = ln.split("\t")[0].encode()
        if name not in seen:
            seen.add(name)
            sizes += [len(x) + 1 for x in by[name]] + [0]
    return [sum(sizes[i:i + 64]) for i in range(0, len(sizes), 64)]


def lines_batch():
    """80 runs (1M1I forty times) on names of 1, 95, 97 and 300 bytes: a wave's 64 lines below and above BED_STAGE; short sequences in
    between (a wave whose runs belong to two sequences); runs of 1, 2, 5 and 40 bases for min_size; coordinates of 1, 7 and 8 digits"""
    b = Batch("bed_lines")
    for n in LINE_NAMES:
        b.add("1M1I" * 40 + "1M", None, dict(), qs=2, qname="N" * n, tname="T", ts=0, tlen=100)
        b.add("2M1I5M2I40M", None, dict(), qs=1, qname="s%d" % n, tname="T", ts=0, tlen=100)
    for at in (9_999_990, 99_999_990):  # ..., 9 999 999, 10 000 000: seven and eight digits
        b.add("1M1I" * 40 + "1M", None, dict(), qs=at, qname="far%d" % at, tname="T", ts=0, tlen=100)
    return b


LINE_OPTS = (dict(), dict(min_size=2), dict(min_size=6), dict(min_size=41), dict(min_size=10 ** 9), dict(exclude_aligned=True), dict(exclude_unaligned=True),
             dict(exclude_aligned=True, exclude_unaligned=True), dict(exclude_unaligned=True, min_size=40), dict(binary=True), dict(binary=True, min_size=2))


def ten_digit_batch():
    """coordinates of ten digits: one sequence of a little over 10^9 bases"""
    b = Batch("bed_ten_digits")
    b.add("1M1I" * 40 + "1M", None, dict(), qs=999_999_990, qname="giga", tname="T", ts=0, tlen=100)
    return b


# ---- group 11: the median of k_cov_merge ----
def median_batch():
    """tile visits by descending score: layers first (high scores), probes last. A probe's level is the smallest L with
    #(its bases whose new count <= L) >= aligned / 2.0"""
    b = Batch("median")
    sc = [10 ** 6]

    def rec(name, qs, cg, qlen, strand="+"):
        sc[0] -= 1
        b.add(cg, None, dict(), qs=qs, qlen=qlen, qname=name, tname="T", ts=0, tlen=10 ** 7, strand=strand, score=sc[0])

    # counts under the probe (before it): a probe of n bases over counts c meets new counts c + 1
    for name, under in (("one", [4]), ("two_meets", [0, 2]), ("two_equal", [2, 2]), ("three_misses", [0, 2, 2]), ("three_meets", [0, 0, 2]),
                        ("four_meets", [0, 0, 2, 2]), ("four_misses", [0, 2, 2, 2]), ("four_late", [0, 1, 2, 3])):
        for i, c in enumerate(under):
            for _ in range(c):
                rec("m_" + name, 10 + i, "1M", 100)
    for name, under in (("one", [4]), ("two_meets", [0, 2]), ("two_equal", [2, 2]), ("three_misses", [0, 2, 2]), ("three_meets", [0, 0, 2]),
                        ("four_meets", [0, 0, 2, 2]), ("four_misses", [0, 2, 2, 2]), ("four_late", [0, 1, 2, 3])):
        rec("m_" + name, 10, "%dM" % len(under), 100, "-")
    # three slices with level ranges of their own: 1 layer on slice 0, 5 on slice 1, 9 on slice 2; the probe covers 20 000 bases of each side slice
    for s, depth in enumerate((1, 5, 9)):
        for _ in range(depth):
            rec("m_slices", s * COV_SLICE, "%dM" % COV_SLICE, 3 * COV_SLICE)
    rec("m_slices", COV_SLICE - 20000, "%dM" % (COV_SLICE + 40000), 3 * COV_SLICE)
    rec("m_slices", COV_SLICE - 2, "%dM" % (COV_SLICE + 3), 3 * COV_SLICE, "-")  # two bases, a whole slice and one base: three level ranges
    rec("m_slices", COV_SLICE - 1, "%dM" % (COV_SLICE + 2), 3 * COV_SLICE)
    # a staircase of 100 steps: the probe over it meets 101 levels (more than a wave's 64, fewer than 256)
    for k in range(100):
        rec("m_stairs", 10 * k, "2000M", 5000)
    rec("m_stairs", 0, "3000M", 5000)
    rec("m_stairs", 5, "990M", 5000, "-")
    return b


# ---- the sets ----
_SETS = {}


def error_free_batches():
    if "ok" not in _SETS:
        _SETS["ok"] = _error_free_batches()
    return _SETS["ok"]


def failing_batches():
    if "bad" not in _SETS:
        _SETS["bad"] = negative_wrap_batches() + error_batches()
    return _SETS["bad"]


def _error_free_batches():
    return (alignment_batches() + [threshold_batch()] + straddle_batches() + serial_batches() + [degenerate_batch()] + window_batches() + [boundary_batch(g) for g in SHAPES]
            + [runs_batch(), lines_batch(), median_batch()])


# ---- for the soak (tools/fuzz_gpu.py): a cigar with the forms its random streams lack ----
def odd_cigar(rng):
    """(cigar text, query bases, target bases): digitless ops, numbers with leading zeros and of eight and more digits, now and then in a
    cigar long enough for the four-wave shape"""
    parts = [filler(rng.choice([0, 2, 30, 500, 1020, 2046, 4090]), rng.randrange(4))]
    for _ in range(rng.choice([1, 2, 5])):
        parts.append(rng.choice(["M", "I", "D", "MI", "0M", "007M", "0001000M", "00000100M", "000000100M", str((1 << 56) + 10) + "M", "1M1I" * rng.choice([3, 256, 512]),
                                 "1MMI", "5=3X"]))
        parts.append(filler(rng.choice([0, 2, 17, 300, 1500]), rng.randrange(4)))
    cg = "".join(parts) or "1M"
    if rng.random() < 0.3:
        cg = to_shape(cg, 256, pad=rng.choice(["0I0D", filler(10)])) if len(cg) <= COV_WAVE_BYTES else cg
    q, t, _ = spans(cg)
    return cg, q, t
