"""The leaf matrix (tests/leafmatrix.py) on the CPU: every case gives its
expected verdicts on the host emulator (the interpreter's own sources built
for x86) and on oracle/c (the reference alone, no kernel source); the inputs
meet the conditions that make a wrong generator visible (computed from the
oracle's values alone); every promised class x width x kind exists; and the
declared asm eligibility is isa.asm_eligible's.  tests/test_gpu_leafmatrix.py
runs the same cases on every device engine.
"""
from collections import defaultdict

import pytest

from mythril_amd import hostemu, isa
from oracle import cdag
from tests import leafmatrix as lm
from tests.opmatrix import _flips


@pytest.fixture(scope="module")
def cases():
    return lm.cases()


def _base(c):
    """a case's name (class/width/label/range[/seed][/flip]) without its
    range, seed and flip: the leaf it tests"""
    parts = c.name.split("/")
    assert parts[3] == c.range and all(x.startswith(("seed", "flip")) for x in parts[4:]), c.name
    return "/".join(parts[:3])


def test_matrix_shape(cases):
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        p = c.program
        assert _base(c) == f"{c.cls}/w{c.width}/" + c.name.split("/")[2], c.name
        assert c.n <= lm.NP and c.expect in (0, 1) and len(c.tuples) == lm.NP, c.name
        assert c.seed >> 32 and c.seed & 0xFFFFFFFF and c.seed >> 32 != c.seed & 0xFFFFFFFF or c.seed == lm.DEFAULT_SEED
        assert len(p.pool) <= lm.POOL_WORDS_MAX, (c.name, len(p.pool))
        # the compiled program's leaves: the declared specs under test, and e of the pinned kind
        got = cdag.program_specs(p)
        for nm, sp in got.items():
            if nm in c.specs:
                want = c.specs[nm]
                assert sp == dict(want, pool=want["pool"] or None), (c.name, nm)
            else:
                assert nm.startswith("e") and len(sp["pool"]) == lm.NP and None not in sp["pool"], (c.name, nm)
                assert (sp["shift"], sp["bits"], sp["hashed"], sp["stride"]) == (0, 8, False, 0), (c.name, nm)
        assert set(c.specs) == set(c.under_test) and set(c.under_test) <= set(got), c.name
        kinds = {int(p.leaves[i * isa.LEAF_WORDS + isa.LEAF_KIND]) for i, n in enumerate(p.leaf_nodes)
                 if n.name in c.specs}
        assert kinds == c.kinds, (c.name, kinds)


def test_promised_cases_exist(cases):
    have = {(c.cls, c.width, k) for c in cases if c.expect for k in c.kinds}
    for row in lm.PROMISED:
        assert row in have, row
    rnd = [c for c in cases if c.cls == "random"]
    for w in lm.WIDTHS:
        here = [c for c in rnd if c.width == w and c.seed == lm.SEED]
        salts = {s["id"] for c in here for s in c.specs.values()}
        assert {0, 0xFFFFFFFF} < salts and len(salts) == 3, w
        assert {c.name.rsplit("flip", 1)[1] for c in here if not c.expect} == {str(f) for f in _flips(w)}, w
        if w != 8:   # the base launch ranges, one program each (8 bits: leafmatrix's docstring)
            assert set(lm.BASE_RANGES) <= {c.range for c in here if c.expect}, w
    assert {c.width for c in rnd if c.seed == lm.DEFAULT_SEED} >= {32, 33, 129, 256}
    for cls, want in (("field", lm.FIELDS), ("interleaved", lm.INTERLEAVED)):
        got = {((s["shift"], s["bits"]) + ((s["stride"],) if cls == "interleaved" else ()))
               for c in cases if c.cls == cls for s in c.specs.values()}
        assert set(want) <= got, (cls, set(want) - got)
    for cls in ("field", "interleaved"):   # the one-entry pool, a constant and a RANDOM entry
        one = [s["pool"] for c in cases if c.cls == cls for s in c.specs.values() if not s["bits"]]
        assert [None] in one and any(p != [None] for p in one), cls
    hashed = [c for c in cases if c.cls == "hashed"]
    assert {s["bits"] for c in hashed for s in c.specs.values()} >= set(lm.HASHED_BITS)
    assert any(len(c.specs) == 2 and len({s["id"] for s in c.specs.values()}) == 2
               and len({s["bits"] for s in c.specs.values()}) == 1 for c in hashed)
    assert any(s["id"] == 0xFFFFFFFF for c in hashed for s in c.specs.values())
    for cls in ("field", "interleaved", "hashed"):   # pool contents
        pools = [(s["width"], s["pool"]) for c in cases if c.cls == cls for s in c.specs.values() if s["bits"]]
        assert any(all(e is None for e in p) for _, p in pools), cls
        assert any(None not in p for _, p in pools), cls
        assert any(None in p and any(e is not None for e in p) for _, p in pools), cls
        assert all((1 << w) - 1 in p for w, p in pools if w < 32 and not all(e is None for e in p)), cls
        wide = [e for w, p in pools if w == 256 for e in p if e is not None]
        assert any(len(set(e.to_bytes(32, "little"))) == 32 for e in wide), cls
    cd = [c for c in cases if c.cls == "calldata"]
    for base in lm.CD_BASES:
        here = [c for c in cd if c.name.split("/")[2] == f"base{base:#x}"]
        assert sum(c.expect for c in here) >= 2
        assert {int(c.name.rsplit("flip", 1)[1]) for c in here if not c.expect} == set(lm.CD_FLIPS)
        for c in here:
            assert "W_CDINS" in c.opcodes() and len(c.program.pool) == 6656, c.name
            size = c.specs["calldatasize"]["pool"]
            for v in (0, 3, 4, 5, base, base + 1, base + 16, base + 31, base + 32, base + 33, 1 << 31, (1 << 32) - 1,
                      1 << 32, (1 << 32) + base + 5, 1 << 255, (1 << 256) - 1, (1 << 255) - 1):
                assert v in size, (c.name, hex(v))
            byte = [s for nm, s in c.specs.items() if nm != "calldatasize"]
            assert len(byte) == 32 and all(len(s["pool"]) == 64 and s["bits"] == 6 and None in s["pool"] for s in byte)
            assert len({(s["shift"], s["id"]) for s in byte}) == 1     # tied to the first
    # W_CDINS takes its index from the instruction below 0x4000 and from the constant pool above
    assert {int(x) & 0xFF for c in cd for x in list(c.program.code)[0::4]} >= {isa.OPCODES["W_CDINS"]}


def test_input_conditions(cases):
    """What makes a wrong generator visible, from the oracle's values alone."""
    digits = defaultdict(list)
    for c in cases:
        vals = [c.tuples[(c.begin + j) & (lm.NP - 1)] for j in range(c.n)]
        for nm, sp in c.specs.items():
            w = sp["width"]
            if not sp["pool"]:
                seen = {m[nm] for m in vals}
                # three quarters of what the launch can hold; one bit needs both values
                assert len(seen) >= max(min(2 ** w, c.n) * 3 // 4, min(2 ** w, 2)), (c.name, nm, len(seen))
                continue
            if not sp["bits"]:
                continue
            ds = [lm.digit(sp, c.seed, c.begin + j) for j in range(c.n)]
            assert len(set(ds)) >= 2, (c.name, nm)
            assert lm.launch_ok(sp, ds), (c.name, nm)     # a wave with gathered and drawn lanes
            digits[(_base(c), nm, sp["bits"])].append(ds)
    assert digits
    for (base, nm, bits), dss in digits.items():
        m = (1 << bits) - 1
        assert lm.bits_seen({"bits": bits}, dss) == (m, m), (base, nm)


def test_sequences_alternate_digit_groups(cases):
    """The draw order, from the programs' LEAF_* instructions."""
    seqs = [c for c in cases if c.cls == "sequence"]
    assert len({c.name.split("/")[2] for c in seqs}) == 5
    for c in seqs:
        g = lm.draw_groups(c.program)
        assert g == c.groups and 4 <= len(c.specs) <= 6, (c.name, g)
        assert len(lm.draw_order(c.program)) == len(c.program.leaf_nodes), c.name    # every leaf drawn once
    by = {c.name.split("/")[2]: c.groups for c in seqs}
    for label in ("stride+shift", "fields"):
        assert "ABA" in by[label] and "DAA" in by[label]      # another group between two members; two in a row
    assert by["random-between"].startswith("ABCA") and by["hashed-salts"].startswith("ABA")
    assert by["tie"] == "AAAAAB"


def test_declared_asm_eligibility(cases):
    for c in cases:
        p = c.program
        assert isa.asm_eligible(p.code, p.leaves, p.consts) == c.asm, c.name
    jc = lm.jit_cases()
    assert len(jc) <= 12 and [c.program for c in jc] == lm.jit_programs()
    assert {k for c in jc for k in c.kinds} == {0, 1, 2, 3}
    assert {c.width for c in jc if c.cls == "random"} == {32, 33, 129, 256}
    for k in (1, 2, 3):
        assert len({c.width for c in jc if c.cls == lm.KINDS[k]} & {32, 33, 129, 256}) >= 2, k
    assert {"sequence", "calldata"} <= {c.cls for c in jc}


def test_host_emulator(cases):
    for c in cases:
        v, _ = hostemu.eval_generated(c.program, c.seed, c.begin, c.n)
        assert lm.first_wrong(c, v) is None, lm.first_wrong(c, v)


def test_reference_alone(cases):
    """oracle/c on the programs' source terms and the declared specs: the
    expected vectors hold without any kernel source."""
    for c in cases:
        specs = dict(cdag.program_specs(c.program), **c.specs)
        _, _, v = cdag.evaluate(c.conj, c.seed, c.begin, c.n, want_verdict=True, specs=specs)
        assert lm.first_wrong(c, v) is None, lm.first_wrong(c, v)


@pytest.mark.parametrize("lds_leaves", [0, lm.JIT_LDS_LEAVES], ids=["literal", "lds_leaves"])
def test_specialised_host_build(lds_leaves):
    """The specialised tier's subset on the x86 build of its generated source."""
    import ctypes

    from mythril_amd import jit
    from tests.test_jit import host_run
    path, names = jit.compile_host(lm.jit_programs(), lds_leaves=lds_leaves)
    # the second build differs: every program with a wide leaf keeps one in an LDS slot
    for c, name in zip(lm.jit_cases(), names):
        src = jit.generate([c.program], [name], "", lds_leaves=lds_leaves)
        wide = any(n.width > isa.NARROW_MAX for n in c.program.leaf_nodes)
        assert ("lds_put8" in src and "lds_get8" in src) == bool(lds_leaves and wide), c.name
    assert any(n.width > isa.NARROW_MAX for c in lm.jit_cases() for n in c.program.leaf_nodes if n.name in c.specs)
    lib = ctypes.CDLL(str(path))
    for c, name in zip(lm.jit_cases(), names):
        v, _ = host_run(lib, name, c.program, c.seed, c.begin, c.n)
        assert lm.first_wrong(c, v) is None, lm.first_wrong(c, v)
