"""Static check of the constant-time signer of signer sets (ssa_k_sign_indexed_ct, schnorr-sig_amd/csrc/ssa_sign.hip):
KeyPair::sign (src/signature.rs:114-129) hashes the public key the key pair holds, so the kernel runs ONE constant-time
base multiplication per signature, [r]G, where ssa_k_sign_ct (PrivateKey::sign) runs two.  Its secret work goes
through the out-of-line functions tests/test_sign_ct_static.py already checks; the key check of the device-form
creation (ct_signer_key) is new and gets the same rules here:
  * no branch on EXEC or VCC, no EXEC narrowing, no v_readfirstlane, v_readlane only to reload a spilled SGPR;
  * every remaining conditional branch follows an s_cmp of an SGPR with an immediate;
  * every call is direct and goes to a checked body;
  * no vector memory access takes its address from a loaded value (the taint pass of tests/test_derive_ct_static.py).
The assembly, its cache and the parsing helpers are those of tests/test_derive_ct_static.py."""
import os
import re
import shutil
import subprocess

import pytest

import test_derive_ct_static as dct

CHECKED = ("ct_load_scalar", "ct_base_mul", "ct_to_aff", "ct_response", "f6_mul_flat", "f6_sqr_flat")
NEW_FUNCS = ("ct_signer_key",)


@pytest.fixture(scope="module")
def fns():
    return dct._functions(dct._asm())


def _calls(body):
    """the targets of the direct calls (s_swappc) of a body, in order, one entry per call"""
    pairs, out = {}, []
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
            assert m.group(1) in pairs, "indirect call through %s" % m.group(1)
            out.append(pairs[m.group(1)])
        else:
            assert not ln.startswith("s_swappc"), ln
    return out


def test_indexed_signer_runs_one_base_multiplication(fns):
    """the point of the feature: ct_base_mul once per signature ([r]G), where ssa_k_sign_ct calls it for sk and r"""
    assert _calls(fns["ssa_k_sign_ct"]).count("ct_base_mul") == 2
    calls = _calls(fns["ssa_k_sign_indexed_ct"])
    assert calls.count("ct_base_mul") == 1, calls
    assert calls.count("ct_load_scalar") == 2, calls          # the nonce and the stored key
    assert {"ct_to_aff", "ct_response"} <= set(calls), calls
    assert set(calls) <= set(CHECKED), calls


def test_device_creation_checks_keys_in_a_checked_function(fns):
    calls = _calls(fns["ssa_k_signer_keys"])
    assert calls == ["ct_signer_key"], calls


def test_new_secret_functions_have_no_data_dependent_control_flow(fns):
    for name in NEW_FUNCS:
        assert name in fns, "function %s not found out of line (inlined? the check needs its own body)" % name
        body = fns[name]
        lines = dct._lines(body)
        assert len(lines) > 20, name
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
        assert set(_calls(body)) <= set(CHECKED + NEW_FUNCS), name
        assert not re.search(r"^\s*s_setpc_b64 (?!s\[30:31\])", body, flags=re.M), name
        assert any(re.match(r"(flat|global)_load", ln) for ln in lines), name
        hits = dct._tainted_addresses(lines)
        assert not hits, "%s: address from loaded data: %s" % (name, hits[:3])


def test_cxx_mirror_declares_the_signer_set(tmp_path):
    """the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) compiles with SignerSet and its methods"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "void f(Context &cx, const std::vector<KeyPair> &kp, Rng rng) {\n"
                   "  SignerSet ss(cx, kp);\n"
                   "  std::vector<std::pair<const uint8_t *, size_t>> msgs;\n"
                   "  std::vector<Signature> a = ss.sign({}, msgs, rng);\n"
                   "  std::vector<KeyedSignature> b = ss.sign_and_bind_pkey({}, msgs, rng);\n"
                   "  std::vector<PublicKey> c = ss.public_keys(); size_t m = ss.size();\n"
                   "  (void)a; (void)b; (void)c; (void)m;\n"
                   "}\n" % root)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
