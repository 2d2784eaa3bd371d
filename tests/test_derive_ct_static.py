"""Static check of the constant-time side of key derivation (schnorr-sig_amd/csrc/ssa_derive.hpp): the reference derives
private children with constant-time HMAC-SHA512, Scalar arithmetic and `conditional_select` on the hardened bit
(src/derivation.rs:88-154), so the code that touches parent keys, chain codes, seeds and child keys must have NO
data-dependent control flow and no data-dependent address.

That code lives in out-of-line functions -- ct_hmac_pads (HMAC key states of a chain code), ct_xprv_prep (parent key
check and the hardened message), ct_xprv_child (one child: message by select, two SHA-512 compressions, masked
arithmetic mod q), ct_master (generate_master_key) -- beside the signer's ct_base_mul / ct_to_aff, which
tests/test_sign_ct_static.py checks.  This test compiles ssa_sign.hip (which includes ssa_derive.hpp) to gfx950 assembly
and asserts in the new bodies the same rules as that test:
  * no branch on EXEC or VCC, no EXEC narrowing, no v_readfirstlane, v_readlane only to reload a spilled SGPR;
  * every remaining conditional branch follows an s_cmp of an SGPR with an immediate (the round counter of SHA-512);
  * every call goes to a checked body;
and in addition that no vector memory access takes its address from a register that holds (or was computed from) a
loaded value: a forward taint pass over each body, with each loop body run again from the state at its back edge."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
CACHE = os.path.join(ROOT, "build", "derive_ct_static")
NEW_FUNCS = ("ct_hmac_pads", "ct_xprv_prep", "ct_xprv_child", "ct_master")
CHECKED_ELSEWHERE = ("ct_load_scalar", "ct_base_mul", "ct_to_aff", "ct_response", "f6_mul_flat", "f6_sqr_flat")


def _asm():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]
    deps.append(os.path.join(ROOT, "include", "schnorr_sig_amd.h"))
    h = hashlib.sha256()
    for p in deps:
        h.update(os.path.basename(p).encode() + b"\0" + open(p, "rb").read() + b"\0")
    os.makedirs(CACHE, exist_ok=True)
    out, stamp = os.path.join(CACHE, "ssa_sign.s"), os.path.join(CACHE, "ssa_sign.s.srchash")
    if not (os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == h.hexdigest()):
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(CSRC, "ssa_sign.hip")], stderr=subprocess.DEVNULL)
        open(stamp, "w").write(h.hexdigest() + "\n")
    return open(out).read()


def _functions(text):
    out = {}
    for ch in re.split(r"^(?=_ZN3ssa\w+:)", text, flags=re.M):
        m = re.match(r"_ZN3ssa(\d+)(\w+):", ch)
        if m:
            out[m.group(2)[:int(m.group(1))]] = ch.split(".Lfunc_end")[0]
    return out


def _lines(body):
    """instructions and branch labels (.LBB*), no directives or comments"""
    out = [ln.split(";")[0].strip() for ln in body.splitlines()]
    return [ln for ln in out if ln and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:$", ln))]


def _vregs(op):
    """VGPR numbers named by one operand: v7, v[4:5]"""
    m = re.fullmatch(r"v(\d+)", op)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def _operands(ln):
    parts = ln.split(None, 1)
    if len(parts) < 2:
        return parts[0], []
    ops = [o.strip() for o in re.split(r",\s*", parts[1])]
    return parts[0], [o.split()[0] for o in ops if o]


def _taint_step(ln, taint, hits):
    op, ops = _operands(ln)
    if not op.startswith("v_") and not re.match(r"(flat|global|buffer|scratch)_", op):
        return
    if re.match(r"(flat|global|buffer|scratch)_load", op):
        addr = set().union(*(_vregs(o) for o in ops[1:])) if len(ops) > 1 else set()
        if addr & taint and ln not in hits:
            hits.append(ln)
        taint |= _vregs(ops[0])
    elif re.match(r"(flat|global|buffer|scratch)_store", op):
        # flat / global: the first operand is the address; scratch: "vdata, vaddr | off, ..."
        addr = _vregs(ops[1]) if op.startswith("scratch") and len(ops) > 1 else _vregs(ops[0]) if ops else set()
        if addr & taint and ln not in hits:
            hits.append(ln)
    elif op.startswith(("v_writelane", "v_readlane", "v_readfirstlane")):
        return
    elif ops:
        dst = _vregs(ops[0])
        src = set().union(*(_vregs(o) for o in ops[1:])) if len(ops) > 1 else set()
        if src & taint:
            taint |= dst
        else:
            taint -= dst


def _tainted_addresses(lines):
    """vector memory instructions whose address VGPRs depend on a value loaded from memory: one forward pass over the
    body (straight-line order), then each loop body once more from the taint state at its back edge"""
    taint, hits, snap = set(), [], []
    for ln in lines:
        _taint_step(ln, taint, hits)
        snap.append(set(taint))
    for i, ln in enumerate(lines):
        m = re.match(r"s_(cbranch_\w+|branch) (\.LBB\d+_\d+)$", ln)
        if m and (m.group(2) + ":") in lines[:i]:
            j = max(k for k in range(i) if lines[k] == m.group(2) + ":")
            t = set(snap[i])
            for x in lines[j:i + 1]:
                _taint_step(x, t, hits)
    return hits


@pytest.fixture(scope="module")
def fns():
    return _functions(_asm())


def test_secret_dependent_derivation_code_has_no_data_dependent_control_flow(fns):
    for name in NEW_FUNCS:
        assert name in fns, "function %s not found out of line (inlined? the check below needs its own body)" % name
        body = fns[name]
        lines = _lines(body)
        assert len(lines) > 100, name
        for bad in ("s_cbranch_execz", "s_cbranch_execnz", "s_cbranch_vccz", "s_cbranch_vccnz", "v_readfirstlane",
                    "s_and_saveexec", "s_andn2_saveexec", "s_xor_saveexec", "s_cbranch_cdbg", "v_cmpx"):
            hits = [ln for ln in lines if bad in ln]
            assert not hits, "%s: %s (%d occurrences), first: %s" % (name, bad, len(hits), hits[0])
        spill = set(re.findall(r"v_writelane_b32 (v\d+),", body))
        for ln in lines:
            if ln.startswith("v_readlane"):
                m = re.match(r"v_readlane_b32 s\d+, (v\d+), \d+$", ln)
                assert m and m.group(1) in spill, (name, ln)
        saved = set()
        for ln in lines:
            m = re.match(r"s_or_saveexec_b64 (s\[\d+:\d+\]), (.+)$", ln)
            if m:
                assert m.group(2) == "-1", (name, ln)
                saved.add(m.group(1))
            elif re.match(r"s_\w+ exec", ln):
                m = re.match(r"s_mov_b64 exec, (s\[\d+:\d+\])$", ln)
                assert m and m.group(1) in saved, (name, ln)
        for i, ln in enumerate(lines):
            if ln.startswith("s_cbranch_scc"):
                prev = [x for x in lines[max(0, i - 400):i] if x.startswith(("s_cmp", "s_and", "s_or", "s_xor", "s_bitcmp"))]
                assert prev and re.match(r"s_cmpk?_(eq|lg|lt|gt|le|ge)_[ui]32 s\d+, (0x[0-9a-f]+|-?\d+)$", prev[-1]), \
                    (name, ln, prev[-3:])
        # calls: direct, and only into checked bodies
        pairs = {}
        for ln in (x.strip() for x in body.splitlines()):
            m = re.match(r"s_add_u32 s(\d+), s\1, _ZN3ssa(\d+)(\w+)@rel32@lo", ln)
            if m:
                pairs["s[%d:%d]" % (int(m.group(1)), int(m.group(1)) + 1)] = m.group(3)[:int(m.group(2))]
                continue
            m = re.match(r"s_mov_b64 (s\[\d+:\d+\]), (s\[\d+:\d+\])$", ln)
            if m and m.group(2) in pairs:
                pairs[m.group(1)] = pairs[m.group(2)]
                continue
            m = re.match(r"s_swappc_b64 s\[30:31\], (s\[\d+:\d+\])$", ln)
            if m:
                assert m.group(1) in pairs, "%s: indirect call through %s" % (name, m.group(1))
                assert pairs[m.group(1)] in NEW_FUNCS + CHECKED_ELSEWHERE, "%s calls %s" % (name, pairs[m.group(1)])
            else:
                assert not ln.startswith("s_swappc"), (name, ln)
        assert not re.search(r"^\s*s_setpc_b64 (?!s\[30:31\])", body, flags=re.M), name


def test_no_load_address_derives_from_loaded_data(fns):
    for name in NEW_FUNCS:
        lines = _lines(fns[name])
        assert any(re.match(r"(flat|global)_load", ln) for ln in lines), name       # the pass has something to track
        hits = _tainted_addresses(lines)
        assert not hits, "%s: address from loaded data: %s" % (name, hits[:3])


def test_taint_pass_catches_a_gather():
    """the checker itself: an address computed from a loaded value is reported, a pointer argument is not"""
    lines = ["flat_load_dwordx2 v[2:3], v[0:1]", "v_lshlrev_b64 v[4:5], 3, v[2:3]", "v_add_co_u32_e32 v6, vcc, v0, v4",
             "v_addc_co_u32_e32 v7, vcc, v1, v5, vcc", "flat_load_dwordx2 v[8:9], v[6:7]"]
    assert _tainted_addresses(lines) == ["flat_load_dwordx2 v[8:9], v[6:7]"]
    assert _tainted_addresses(lines[:1] + ["flat_load_dwordx2 v[8:9], v[0:1] offset:8"]) == []


def test_sha512_uses_alignbit_rotates_and_bfi(fns):
    """the compression as the header describes it: rotates as v_alignbit_b32, Ch / Maj as v_bfi_b32, round constants
    through scalar loads (no vector load of the table)"""
    body = _lines(fns["ct_xprv_child"])
    assert sum(ln.startswith("v_alignbit_b32") for ln in body) >= 2 * 6 * 80
    assert sum(ln.startswith("v_bfi_b32") for ln in body) >= 2 * 16
    assert any(ln.startswith("s_load_dwordx") for ln in body)


def test_kernels_call_the_checked_functions(fns):
    def called(k):
        return {rest[:int(ln)] for _, ln, rest in re.findall(r"(_ZN3ssa(\d+)(\w+))@rel32@lo", fns[k])}
    assert {"ct_xprv_child", "ct_base_mul", "ct_to_aff"} <= called("ssa_k_xprv_derive")
    assert {"ct_xprv_prep", "ct_base_mul", "ct_to_aff", "ct_hmac_pads"} <= called("ssa_k_derive_prep")
    assert "ct_master" in called("ssa_k_xprv_master")
