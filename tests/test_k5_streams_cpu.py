"""The generated K5 instruction streams (rsa_attn_block.h, rsa_attn_block64.h), read back as text on the CPU.

The generators place every `s_waitcnt lgkmcnt(n)` by counting the LDS reads issued behind the one an MFMA needs.  A count that is
one too high is a silent race on the GPU, not a test failure -- so this file re-checks the waits with a model that knows nothing
about the generators: it sees only the macro names and the instruction text.

The model.  LDS reads (`ds_read_*`) complete in issue order; `s_waitcnt lgkmcnt(n)` leaves at most the last n of them
outstanding; an instruction that names a vector register -- as source or destination, `v7` or inside `v[4:7]`; a named asm operand
`%[x]` counts as a register of its own -- may not be issued while an outstanding read still has to write that register.  LDS-DMA
(`global_load_lds_*`) counts on vmcnt and gets no treatment of its own.

Nothing here looks for particular instructions or pins a body: a deliberate schedule change stays an edit of one generator.
"""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rectified_spaattn_amd", "csrc")
DTS = ("BF16", "F16")


def run_generator(*args):
    return subprocess.run([sys.executable, *args], cwd=CSRC, check=True, capture_output=True, text=True).stdout


def parse_macros(text):
    """{name: [instruction text, ...]} of a generated header; a one-line #define (operand lists, clobbers) has no instructions."""
    macros, body = {}, None
    for line in text.split("\n"):
        m = re.match(r"#define (\w+)", line)
        if m:
            assert m.group(1) not in macros, f"{m.group(1)} defined twice"
            body = macros[m.group(1)] = []
        elif body is not None and line.startswith('    "'):
            m = re.fullmatch(r'    "(.*)\\n\\t"( \\)?', line)
            assert m, line
            body.append(m.group(1))
        if not line.endswith("\\"):
            body = None
    return macros


@pytest.fixture(scope="module")
def headers():
    return {"block": parse_macros(run_generator("gen_k5_block.py")), "block64": parse_macros(run_generator("gen_k5_block64.py"))}


def streams(headers, family):
    """(name, instructions) of every macro of both headers that has a body and `family` in its name"""
    return [(n, b) for h in headers.values() for n, b in h.items() if family in n and b]


# ---------------------------------------------------------------------------------------------------------------------
# the wait-discipline model
# ---------------------------------------------------------------------------------------------------------------------
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]|(%\[\w+\])")
WAIT = re.compile(r"lgkmcnt\((\d+)\)")


def registers(text):
    regs = set()
    for one, lo, hi, named in REG.findall(text):
        regs |= {named} if named else {int(one)} if one else set(range(int(lo), int(hi) + 1))
    return regs


def decode(lines):
    """per instruction: (text, counted wait or None, registers it names, registers an LDS read among them will write)"""
    prog = []
    for t in lines:
        w = WAIT.search(t) if t.startswith("s_waitcnt") else None
        prog.append((t, int(w.group(1)) if w else None, registers(t),
                     registers(t.split(",")[0]) if t.startswith("ds_read") else None))
    return prog


def check(prog, bump=None):
    """Run the model over a decoded stream (bump: index of a wait whose count is raised by one).
    -> (violations as (index, text), number of reads outstanding at the end)"""
    flying, bad = [], []          # flying: destination sets of the outstanding reads, oldest first
    for i, (text, wait, regs, dest) in enumerate(prog):
        if wait is not None:
            n = wait + (i == bump)
            flying = flying[len(flying) - n:] if n < len(flying) else flying
            continue
        if any(regs & f for f in flying):
            bad.append((i, text))
        if dest is not None:
            flying.append(dest)
    return bad, len(flying)


def test_model_on_hand_written_streams():
    """the model itself: it accepts a covered read, and flags an uncovered one, a late wait and a read left flying"""
    ok = ["ds_read_b128 v[4:7], v20", "ds_read_b64 v[8:9], v21 offset:64", "s_waitcnt lgkmcnt(1)", "v_add_f32 v1, v5, v1",
          "s_waitcnt lgkmcnt(0)", "v_mfma_f32_32x32x16_bf16 v[32:47], v[6:9], a[0:3], v[32:47]"]
    assert check(decode(ok)) == ([], 0)
    assert check(decode(ok), bump=2)[0] == [(3, ok[3])]                    # v5 is still being written
    assert check(decode(ok), bump=4)[0] == [(5, ok[5])]                    # v[8:9] overlaps v[6:9]
    assert check(decode(ok[:4])) == ([], 1)                                # the second read is never waited for
    assert check(decode(["ds_read_u16 %[lv], %[la]", "v_readfirstlane_b32 s87, %[lv]"]))[0]
    assert check(decode(["ds_read_u16 %[lv], %[la]", "v_add_u32 %[la], 2, %[la]", "s_waitcnt vmcnt(0)"])) == ([], 1)


def test_blocks_wait_for_every_read(headers):
    blocks = streams(headers, "_BLOCK")
    assert len(blocks) == 100
    for name, body in blocks:
        bad, left = check(decode(body))
        assert not bad, f"{name}: issued while an LDS read still has to write its register: {bad[:3]}"
        assert left == 0, f"{name}: {left} LDS reads outstanding at the end of the statement"


def test_loops_wait_for_every_read(headers):
    """straight-line scan (the loop statements contain branches: every path the scan does not take is left to the GPU tests)"""
    loops = streams(headers, "_LOOP")
    assert len(loops) == 8
    for name, body in loops:
        bad, _ = check(decode(body))
        assert not bad, f"{name}: issued while an LDS read still has to write its register: {bad[:3]}"


def test_no_block_wait_could_be_one_higher(headers):
    """Sensitivity: raising ANY single counted wait of a block by one makes the model object -- so no wait is looser than the
    model can see, and the model is not blind to any of them.  Exhaustive over every wait of every *_BLOCK* macro of both
    headers (every dtype, every form): no sampling.  The *_LOOP* macros are left out: a linear scan is no sound model across
    their branches, and a mutant behind one would pass unseen."""
    mutants = missed = 0
    for name, body in streams(headers, "_BLOCK"):
        prog, before = decode(body), mutants
        for i, (_, wait, _, _) in enumerate(prog):
            if wait is None:
                continue
            mutants += 1
            bad, left = check(prog, bump=i)
            if not bad and left == 0:
                missed += 1
                print(f"{name}: instruction {i}, lgkmcnt({wait}) -> ({wait + 1}) goes unnoticed")
        assert mutants > before, f"{name}: no counted wait found"
    print(f"{mutants - missed} of {mutants} single-wait mutants caught")
    assert missed == 0


# ---------------------------------------------------------------------------------------------------------------------
# the 64-row generator keeps no head dim in module state
# ---------------------------------------------------------------------------------------------------------------------
def load_generator():
    """a fresh module object of gen_k5_block64.py, imported by path"""
    spec = importlib.util.spec_from_file_location("gen_k5_block64_under_test", os.path.join(CSRC, "gen_k5_block64.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, CSRC)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(CSRC)
    return mod


def test_head_dims_do_not_leak_into_each_other(headers):
    """head dim 64 then 128 in one process = 128 then 64 = one process each = the header the command line prints"""
    one = "import gen_k5_block64 as g; print(g.main_one(g.HEAD_DIMS[{}]))"
    apart = [parse_macros(run_generator("-c", one.format(i))) for i in (0, 1)]
    g = load_generator()
    assert [c.D for c in g.HEAD_DIMS] == [128, 64]
    backward = [parse_macros(g.main_one(c)) for c in reversed(g.HEAD_DIMS)][::-1]
    g = load_generator()
    forward = [parse_macros(g.main_one(c)) for c in g.HEAD_DIMS]
    for i, what in enumerate(("head dim 128", "head dim 64")):
        assert apart[i].keys() == forward[i].keys() == backward[i].keys(), what
        for name in apart[i]:
            assert apart[i][name] == forward[i][name] == backward[i][name], f"{what}: {name} depends on what was generated before it"
    assert {**apart[0], **apart[1]} == headers["block64"]
    with pytest.raises(AttributeError):     # the configuration is immutable
        g.HEAD_DIMS[0].D = 64


# ---------------------------------------------------------------------------------------------------------------------
# the macros the kernels name
# ---------------------------------------------------------------------------------------------------------------------
def names(pattern, **ranges):
    """pattern.format over the product of the ranges"""
    out = [{}]
    for key, values in ranges.items():
        out = [dict(d, **{key: v}) for d in out for v in values]
    return {pattern.format(**d) for d in out}


def test_macro_names(headers):
    block = set()
    # the 2-byte 32-row kernel: -m form at head dim 128, classic form at 64; K/V slot parity x sub-step parity
    block |= names("RSA_K5_BLOCKN_128_{dt}_V{v}_S{s}", dt=DTS, v=range(2), s=range(2))
    block |= names("RSA_K5_BLOCK_64_{dt}_V{v}_S{s}", dt=DTS, v=range(2), s=range(2))
    block |= names("RSA_K5_{what}{tag}", what=("OPS", "CLOBBER"), tag=("N_128", "_64"))
    # the e4m3 kernel: exp / code-map / code-map + DMA at head dim 128, code-map (+ DMA) at 64; ring slot T
    block |= names("RSA_K5F8_BLOCK{form}_T{t}", form=("", "C", "CD", "C64", "CD64"), t=range(4))
    block |= names("RSA_K5F8_{what}", what=("OPS", "OPSD", "CLOBBER", "OPS64", "OPS64D", "CLOBBER64"))
    # its pv form: tile % 6
    block |= names("RSA_K5F8H{hd}_BLOCK{dma}_{dt}_T{t}", hd=("", "64"), dma=("", "D"), dt=DTS, t=range(6))
    block |= names("RSA_K5F8H{hd}_{what}", hd=("", "64"), what=("OPS", "OPSD", "CLOBBER"))
    assert set(headers["block"]) == block

    block64 = set()
    for pfx in ("RSA_K5W_", "RSA_K5V_"):      # head dim 128, head dim 64
        block64 |= names(pfx + "BLOCK_{dt}_U{u}", dt=DTS, u=range(4))
        block64 |= names(pfx + "{what}_{dt}", what=("LOOP", "QK0"), dt=DTS) | names(pfx + "LOOP_{dt}_R256", dt=DTS)
        block64 |= names(pfx + "{ops}{what}_{s}", ops=("", "OPS_"), what=("ROWMAX", "MASK", "RESCALE"), s="AB")
        block64 |= names(pfx + "{ops}NMZERO", ops=("", "OPS_")) | {pfx + "OZERO"}
        block64 |= names(pfx + "QWRITE_H{h}_K{k}", h=range(2), k=range(8)) | names(pfx + "OREAD_H{h}_D{d}", h=range(2), d=range(4))
        block64 |= names(pfx + "OPS{what}", what=("", "_LOOP", "_QK0")) | names(pfx + "CLOBBER_{what}", what=("TMP", "O", "Q", "LOOP"))
    assert set(headers["block64"]) == block64
