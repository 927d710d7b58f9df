"""The device FASTA index (fasta_kernel.h: k_fa_count / k_fa_scan / k_fa_write / k_fa_records) against the checker's reader
(tests/faffy_lib.py, host/paffy_cmds.c:fasta_read) on adversarial text, and on one sequence whose text passes 2^32 bytes."""
import hashlib
import random

import pytest

import faffy_lib as F

pytestmark = pytest.mark.gpu

TILE = 65536


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def check(eng, files):
    got = eng.fasta_records(files)
    want = F.fasta_read_files(files)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {k}"


def noisy_file(rnd, size, headers=True):
    """lines of bases, spaces, tabs, '\\r' inside and at the end, blank lines, CRLF, headers with spaces and '\\r'"""
    out = bytearray()
    while len(out) < size:
        r = rnd.random()
        if headers and r < 0.05:
            out += b">" + bytes(rnd.choice(b"ab |\t\r x1") for _ in range(rnd.randrange(0, 12))) + rnd.choice([b"\n", b"\r\n", b"\r\r\n"])
        elif r < 0.1:
            out += rnd.choice([b"\n", b"\r\n", b" \n", b"\t\r\n", b"\r\r\r\n"])
        else:
            n = rnd.choice([1, 7, 60, 61, 255, 256, 257, 3000])
            line = bytes(rnd.choice(b"ACGTNacgtn  \t\r") for _ in range(n))
            out += line + rnd.choice([b"\n", b"\r\n", b"\r\r\n", b"\n"])
    return bytes(out)


def test_small_known_answers(eng):
    check(eng, [b">a\nACGT\n"])
    check(eng, [b">a\r\nAC\r\nGT\r\n>b\n\n>c\nA C\tG\n"])
    check(eng, [b">only\n>headers\n>here"])
    check(eng, [b"no header at all\nACGT\n"])
    check(eng, [b">a\nAC", b"GG\nTT\n>b\nT\n"])  # 1st file without a final '\n'; text before the 2nd file's first header
    check(eng, [b"", b">a\nA\r", b"", b"\r\n>b\nC\r\r", b"\n"])  # empty files; '\r' runs that end a file


def test_cr_runs_across_tile_and_span_boundaries(eng):
    for at in (TILE, 2 * TILE, 256, 512, 4096):
        for shift in range(-4, 5):
            body = bytearray(b"A" * (3 * TILE))
            p = at + shift - 3
            body[p:p + 6] = b"\r\r\r\r\r\r"
            body[p + 6] = ord(b"\n") if shift % 2 else ord(b"C")  # the run ends its line, or stays inside it
            check(eng, [b">x\n" + bytes(body) + b"\n"])


def test_adversarial_seeded(eng):
    rnd = random.Random(11)
    files = [noisy_file(rnd, 300_000), b"junk before\nACGT\r\n" + noisy_file(rnd, 200_000), noisy_file(rnd, 70_000, headers=False),
             noisy_file(rnd, 150_000)]
    files[0] = files[0].rstrip(b"\n")  # the 1st file ends without '\n'
    check(eng, files)
    # file boundaries at every alignment around a tile edge
    for cut in range(TILE - 20, TILE + 20, 3):
        text = files[1][: 2 * TILE]
        check(eng, [text[:cut], text[cut:]])


def test_megabase_single_line(eng):
    rnd = random.Random(3)
    line = bytes(rnd.choice(b"ACGT \t\r") for _ in range(1_000_000))
    check(eng, [b">long header line\r\n" + line + b"\r\n>next\nAC\n"])
    check(eng, [b">" + line + b"\nACGT\n"])  # a header longer than a tile


def test_sequence_text_past_4gib(eng):
    """one record of 64-byte CRLF lines (62 bases) whose text passes 2^32 bytes, generated on the device; per-chunk SHA-256 of the
    compact bases against the same bytes taken from a torch view of the text"""
    import torch

    dev = eng.device
    n_lines = (1 << 32) // 64 + 4099
    hdr = b">big\n"
    total = len(hdr) + n_lines * 64
    text = torch.empty(total + 32, dtype=torch.uint8, device=dev)
    text[: len(hdr)] = torch.tensor(list(hdr), dtype=torch.uint8, device=dev)
    body = text[len(hdr): len(hdr) + n_lines * 64].view(n_lines, 64)
    lut = torch.tensor(list(b"ACGTNacgtn"), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    step = 1 << 22
    for r0 in range(0, n_lines, step):
        r1 = min(n_lines, r0 + step)
        idx = torch.randint(0, 10, (r1 - r0, 62), device=dev, generator=g, dtype=torch.int64)
        body[r0:r1, :62] = lut[idx]
        del idx
    body[:, 62] = 13
    body[:, 63] = 10
    torch.cuda.synchronize()
    n_rec, n_bases = eng.fasta_index(text, total, [0])
    assert (n_rec, n_bases) == (1, n_lines * 62)
    assert eng.fasta_table() == [(1, 3, 0, n_lines * 62)]
    got = torch.empty(n_bases, dtype=torch.uint8, device=dev)
    eng.fasta_bases(0, n_bases, got)
    for r0 in range(0, n_lines, step):
        r1 = min(n_lines, r0 + step)
        want = hashlib.sha256(body[r0:r1, :62].contiguous().cpu().numpy().tobytes()).hexdigest()
        have = hashlib.sha256(got[r0 * 62: r1 * 62].cpu().numpy().tobytes()).hexdigest()
        assert have == want, f"lines {r0}..{r1}"
    del got, body, text
    torch.cuda.empty_cache()
