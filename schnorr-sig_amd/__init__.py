"""schnorr_sig_amd -- host-side mirror of toposware/schnorr-sig's verification API over the
MI355X-native HIP engine (C ABI: include/schnorr_sig_amd.h).

This package is plumbing only: it loads csrc/libschnorr_sig_amd.so with ctypes and forwards
to it.  There is no CPU compute path; if the HIP library is missing, import fails loudly.

Reference API mirrored (names and semantics, reference file:line):
  Signature.verify(message, pkey)            src/signature.rs:181-205
  PublicKey.verify_signature / KeyPair.verify_signature   src/signature.rs:159-176
  KeyPair.new / KeyPair.sign / sign_and_bind_pkey   src/keypair.rs:57-65, src/signature.rs:114-156
  PublicKey.to_bytes / from_bytes            src/public.rs:49-56
  KeyedSignature.to_bytes / from_bytes       src/signature.rs:236-271
  verify_batch(signatures, public_keys, messages, rng)    src/batch.rs:31-50
  SignatureError.{InvalidPublicKey, InvalidSignature}     src/error.rs:13-31
  *_LENGTH constants                         src/constants.rs:12-30
  ChainCode / ExtendedPrivateKey / ExtendedPublicKey, PrivateKey.derive_private, PublicKey.derive_public
                                             src/derivation.rs:30-317

The directory is named `schnorr-sig_amd`; import it as `schnorr_sig_amd` (repo-root shim).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SSA_LIB: an alternative build of the same library (kernel experiments, tools/build_variants.sh); default: in-tree
LIB_PATH = os.environ.get("SSA_LIB") or os.path.join(_HERE, "csrc", "libschnorr_sig_amd.so")

# src/constants.rs:12-30
SCALAR_LENGTH = 32
PRIVATE_KEY_LENGTH = 32
BASEFIELD_LENGTH = 48
PUBLIC_KEY_LENGTH = 49          # compressed wire form (ssa_compress_many / ssa_decompress_many)
AFFINE_PUBLIC_KEY_LENGTH = 96   # in-memory AffinePoint (x, y): what the engine consumes
KEY_PAIR_LENGTH = 32
SIGNATURE_LENGTH = 81
KEYED_SIGNATURE_LENGTH = 130

OK, INVALID_PUBLIC_KEY, INVALID_SIGNATURE, MALFORMED = 0, 1, 2, 3
ERR_ARG, ERR_HIP, ERR_PARAMS, ERR_NO_DEVICE, ERR_TABLE = -1, -2, -3, -4, -5
TABLE_COMB, TABLE_CT = 0, 1        # ssa_debug_table_read / _xor: the comb for G, the constant-time signer's table
SELFCHECK_FIELDS = ("rows", "bad", "first_bad", "ctab_rows", "ctab_bad", "ctab_first_bad", "builds", "bits")
FLAG_CHECK_TORSION = 1
FLAG_FORCE_LANE = 2   # throughput kernels (one signature per lane) whatever the batch size
FLAG_FORCE_COOP = 4   # low-latency kernel (one wave per signature) whatever the batch size
FLAG_SIG_FLAG_BYTE = 8  # verify_batch's semantics for byte 48 of the signature (src/batch.rs:104)
FLAG_SIGN_CT = 16       # constant-time signing (the reference's `&BASEPOINT_TABLE * r`, src/signature.rs:67,116)
FLAG_SIGN_KEYED = 32    # 130-byte KeyedSignature records out (src/signature.rs:237-245)
AGG_CHECK = 1            # SSA_AGG_CHECK: ssa_aggregate_many screens the signatures first
FLAG_DERIVE_PUBLIC = 64  # xprv -> xpub children (ExtendedPrivateKey::derive_public, src/derivation.rs:160-174)
# src/derivation.rs, src/constants.rs
CHAIN_CODE_LENGTH = 32
EXTENDED_PRIVATE_KEY_LENGTH = 64
EXTENDED_PUBLIC_KEY_LENGTH = 81
PRIVATE_KEY_SEED_LENGTH = 32
DERIVE_NONE = 1          # status of a derivation lane whose CtOption is none
KEYSET_KINDS = {"auto": 0, "comb": 1, "ladder": 2}
_MODE_FLAGS = {None: 0, "auto": 0, "lane": FLAG_FORCE_LANE, "coop": FLAG_FORCE_COOP}

Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF


class _DeviceRng:
    """the `rng` that has the GPU draw the nonces itself (ssa_*_rng): no nonce exists on the
    host.  Accepted by KeyPair.sign / sign_and_bind_pkey, PrivateKey.sign / sign_and_bind_pkey and SignerSet.sign."""

    def __repr__(self):
        return "DEVICE_RNG"

    def __call__(self, n):
        raise TypeError("DEVICE_RNG draws on the device only; it yields no bytes on the host")


DEVICE_RNG = _DeviceRng()


class SignatureError(Exception):
    """src/error.rs:13-31 (Display strings kept verbatim)."""
    InvalidPublicKey = "InvalidPublicKey"
    InvalidSignature = "InvalidSignature"
    _MSG = {
        "InvalidPublicKey": "The public key is not an element of the prime subgroup.",
        "InvalidSignature": "The signature is invalid or was incorrectly computed.",
    }

    def __init__(self, kind):
        super().__init__(self._MSG[kind])
        self.kind = kind

    def __repr__(self):
        return "Err(%s)" % self.kind


class MalformedInput(ValueError):
    """Inputs on which the reference panics (src/signature.rs:186, src/batch.rs:37-44,67)."""


HIP_RUNTIME_BOUND = None      # path of the HIP runtime this module loaded ahead of the library, or a note why none was


def _share_hip_runtime_with_torch():
    """ONE HIP runtime per process.  PyTorch-ROCm wheels carry their own libamdhip64.so (SONAME libamdhip64.so.7) and
    ask for it as `libamdhip64.so`; this library asks for `libamdhip64.so.7`.  With torch imported first the loader
    gives us torch's copy (SONAME match); the other way round torch's name does not match /opt/rocm's copy, a second
    runtime is loaded and finds no device ("No HIP GPUs are available").  A process that will use both (device tensors
    handed to the *_device entry points) must share one: when torch is installed and not imported yet, its copy is
    loaded first.  ONLY libamdhip64.so is loaded -- its RPATH brings torch's own HSA runtime with it; loading the two
    separately and ignoring a failure could bind the system HIP runtime to torch's HSA (or the reverse), a version mix
    that only shows as a GPU initialisation failure much later.  What was bound is kept in HIP_RUNTIME_BOUND (bench.py
    prints it); a failure is a warning, not silence.  SSA_NO_TORCH_HIP_PRELOAD=1 turns this off (a process that never
    imports torch does not need it)."""
    global HIP_RUNTIME_BOUND
    import sys
    if "torch" in sys.modules:
        HIP_RUNTIME_BOUND = "torch was imported first: its runtime serves both (SONAME match)"
        return
    if os.environ.get("SSA_NO_TORCH_HIP_PRELOAD"):
        HIP_RUNTIME_BOUND = "system runtime (SSA_NO_TORCH_HIP_PRELOAD)"
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        HIP_RUNTIME_BOUND = "system runtime (torch is not installed)"
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(path):
        HIP_RUNTIME_BOUND = "system runtime (torch carries no libamdhip64.so)"
        return
    try:
        C.CDLL(path, mode=C.RTLD_GLOBAL)
        HIP_RUNTIME_BOUND = path
    except OSError as exc:       # not loadable here (no ROCm userland around it): the system runtime serves
        import warnings
        HIP_RUNTIME_BOUND = "system runtime (torch's copy did not load: %s)" % exc
        warnings.warn("schnorr_sig_amd: torch's HIP runtime %s did not load (%s); importing torch later in this process "
                      "will bring a second runtime" % (path, exc))


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "schnorr_sig_amd: HIP library %s is missing; run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, sz, u32, u64p, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint64), C.c_int
    sigs = {
        "ssa_ctx_create": (i32, [C.POINTER(vp), i32, vp, sz]),
        "ssa_ctx_create_ex": (i32, [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]),
        "ssa_ctx_info": (i32, [vp, u64p]),
        "ssa_pubkey_many": (i32, [vp, vp, sz, vp]),
        "ssa_pubkey_many_device": (i32, [vp, vp, sz, vp]),
        "ssa_ctx_destroy": (None, [vp]),
        "ssa_strerror": (C.c_char_p, [i32]),
        "ssa_default_params": (vp, []),
        "ssa_ctx_set_stream": (i32, [vp, vp]),
        "ssa_ctx_uses_default_params": (i32, [vp]),
        "ssa_ctx_sync": (i32, [vp]),
        "ssa_ctx_enable_timing": (i32, [vp, i32]),
        "ssa_ctx_read_timing": (i32, [vp, C.c_char_p, C.POINTER(C.c_double), u64p]),
        "ssa_verify": (i32, [vp, vp, vp, vp, sz, u32]),
        "ssa_verify_many": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_verify_batch": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32]),
        "ssa_hash_message_many": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_rescue_hash_many": (i32, [vp, vp, u32, sz, vp]),
        "ssa_keygen_sign_many": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp, vp]),
        "ssa_verify_many_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_hash_message_many_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_rescue_hash_many_device": (i32, [vp, vp, u32, sz, vp]),
        "ssa_keygen_sign_many_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp, vp]),
        "ssa_verify_batch_msm": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_verify_batch_msm_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u32, vp]),
        "ssa_verify_keyed_many": (i32, [vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_keyset_create": (i32, [vp, vp, vp, sz, u32, C.POINTER(vp)]),
        "ssa_keyset_create_device": (i32, [vp, vp, vp, sz, u32, C.POINTER(vp)]),
        "ssa_keyset_destroy": (None, [vp]),
        "ssa_keyset_status": (i32, [vp, vp]),
        "ssa_verify_many_indexed": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_verify_many_indexed_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_multi_create": (i32, [C.POINTER(vp), C.POINTER(i32), i32, vp, sz]),
        "ssa_multi_destroy": (None, [vp]),
        "ssa_multi_verify_many": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_multi_verify_batch_msm": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_decompress_many": (i32, [vp, vp, sz, vp, vp, vp]),
        "ssa_decompress_many_device": (i32, [vp, vp, sz, vp, vp, vp]),
        "ssa_debug_arith": (i32, [vp, i32, vp, vp, sz, sz, sz, vp, sz]),
        "ssa_bench_fpmul": (i32, [vp, i32, C.POINTER(C.c_double)]),
        "ssa_debug_chacha20": (i32, [vp, vp, vp, u32, sz, vp]),
        "ssa_verify_batch_msm_partial_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u32, vp]),
        "ssa_verify_batch_msm_partial": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp]),
        "ssa_msm_combine_device": (i32, [vp, vp, sz, vp]),
        "ssa_msm_combine": (i32, [vp, vp, sz]),
        "ssa_abi_version": (i32, []),
        "ssa_keygen_sign_many_ex": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_keygen_sign_many_ex_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_compress_many": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_compress_many_device": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_ctx_stream_release": (i32, [vp, vp]),
        "ssa_ctx_stream_acquire": (i32, [vp, vp]),
        "ssa_debug_fault_after_chunk": (i32, [vp, i32]),
        "ssa_debug_tail_plan": (i32, [u32, u32, u32, i32, u32, sz, u32, vp]),
        "ssa_debug_split_plan": (i32, [sz, u32, sz, u32, sz, sz, i32, vp]),
        "ssa_debug_split_config": (i32, [vp, C.c_int64, i32, i32, i32]),
        "ssa_debug_split_timing": (i32, [vp, C.c_char_p, vp]),
        "ssa_verify_batch_screened": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p]),
        "ssa_verify_batch_screened_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u32, vp, vp]),
        "ssa_debug_screen_plan": (i32, [sz, u32, vp]),
        "ssa_debug_screen_segments": (i32, [vp, u32]),
        "ssa_verify_many_dedup": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p, vp]),
        "ssa_verify_many_dedup_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]),
        "ssa_verify_many_screened": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p, vp]),
        "ssa_verify_many_screened_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u32, vp, vp, vp]),
        "ssa_keycache_create": (i32, [vp, sz, C.POINTER(vp)]),
        "ssa_keycache_destroy": (None, [vp]),
        "ssa_keycache_clear": (i32, [vp]),
        "ssa_keycache_info": (i32, [vp, u64p]),
        "ssa_verify_many_cached": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p, vp]),
        "ssa_verify_many_cached_device": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u32, vp, vp, vp]),
        "ssa_keycache_create_ex": (i32, [vp, sz, u32, C.POINTER(vp)]),
        "ssa_verify_keyed_many_cached": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p, vp]),
        "ssa_verify_keyed_many_cached_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u32, vp, vp, vp]),
        "ssa_verify_keyed_many_device": (i32, [vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_debug_keycache_plan": (i32, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(u32)]),
        "ssa_keycache_set_eviction": (i32, [vp, u32]),
        "ssa_keycache_eviction_info": (i32, [vp, u64p]),
        "ssa_debug_keycache_keep": (i32, [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]),
        "ssa_debug_dedup_device": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_debug_dedup_config": (i32, [vp, C.c_double, u32]),
        "ssa_xprv_master_many": (i32, [vp, vp, sz, vp, vp]),
        "ssa_xprv_master_many_device": (i32, [vp, vp, sz, vp, vp]),
        "ssa_xprv_derive_many": (i32, [vp, vp, sz, vp, vp, sz, u32, vp, vp]),
        "ssa_xprv_derive_many_device": (i32, [vp, vp, sz, vp, vp, sz, u32, vp, vp]),
        "ssa_xpub_derive_many": (i32, [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "ssa_xpub_derive_many_device": (i32, [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "ssa_debug_hmac_sha512": (i32, [vp, vp, sz, vp, sz, sz, vp]),
        "ssa_signer_set_create": (i32, [vp, vp, sz, C.POINTER(vp)]),
        "ssa_signer_set_create_device": (i32, [vp, vp, sz, sz, C.POINTER(vp)]),
        "ssa_signer_set_destroy": (None, [vp]),
        "ssa_signer_set_status": (i32, [vp, vp]),
        "ssa_signer_set_public_keys": (i32, [vp, vp, vp]),
        "ssa_sign_many_indexed": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp]),
        "ssa_sign_many_indexed_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_ctx_selfcheck": (i32, [vp, u32, u64p]),
        "ssa_debug_table_read": (i32, [vp, i32, C.c_uint64, C.c_uint64, vp]),
        "ssa_debug_table_xor": (i32, [vp, i32, C.c_uint64, u32, C.c_uint64]),
        "ssa_debug_corrupt_table_builds": (i32, [i32]),
        "ssa_keyset_selfcheck": (i32, [vp, u32, vp, u64p]),
        "ssa_keycache_selfcheck": (i32, [vp, u32, u64p]),
        "ssa_debug_keytab_xor": (i32, [vp, vp, i32, C.c_uint64, u32, C.c_uint64]),
        "ssa_debug_keytab_read": (i32, [vp, vp, i32, C.c_uint64, vp]),
        "ssa_keygen_sign_many_rng": (i32, [vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_keygen_sign_many_rng_device": (i32, [vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_sign_many_indexed_rng": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp]),
        "ssa_sign_many_indexed_rng_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]),
        "ssa_signer_set_generate": (i32, [vp, sz, C.POINTER(vp)]),
        "ssa_signer_set_secret_keys": (i32, [vp, vp]),
        "ssa_debug_pin_rng": (i32, [vp, vp]),
        "ssa_debug_draw_scalars": (i32, [vp, vp, sz, vp]),
        "ssa_debug_poison_workspaces": (i32, [vp, i32]),
        "ssa_aggregate_many": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p]),
        "ssa_aggregate_many_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]),
        "ssa_verify_aggregate": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_verify_aggregate_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_debug_aggregate_coeffs": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_aggregate_shard_tops_device": (i32, [vp, vp, u32, vp, vp, vp, sz, sz, sz, sz, vp, vp]),
        "ssa_aggregate_root_device": (i32, [vp, vp, sz, sz, sz, vp]),
        "ssa_aggregate_shard_fold_device": (i32, [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]),
        "ssa_verify_aggregate_shard_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp, sz, sz, vp, vp]),
        "ssa_aggregate_combine_device": (i32, [vp, vp, sz, vp]),
        "ssa_verify_aggregate_combine_device": (i32, [vp, vp, sz, vp, sz, vp]),
        "ssa_aggregate_many_sliced": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p]),
        "ssa_aggregate_many_sliced_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]),
        "ssa_verify_aggregate_sliced": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_verify_aggregate_sliced_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_multi_aggregate_many": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, u64p]),
        "ssa_multi_verify_aggregate": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_debug_aggregate_shard_coeffs": (i32, [vp, vp, sz, sz, vp]),
        "ssa_aggregate_valid_many": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp]),
        "ssa_aggregate_valid_many_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp]),
        "ssa_aggregate_valid_many_cached": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp, vp, vp, vp]),
        "ssa_aggregate_valid_many_cached_device": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp, vp, vp,
                                                         vp]),
        "ssa_aggregate_valid_keyed_many_cached": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp, vp, vp]),
        "ssa_aggregate_valid_keyed_many_cached_device": (i32, [vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp, vp, vp]),
        "ssa_debug_aggregate_keep": (i32, [vp, vp, sz, vp, u64p]),
        "ssa_verify_aggregates_many": (i32, [vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, vp]),
        "ssa_verify_aggregates_many_device": (i32, [vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, vp]),
        "ssa_debug_aggregates_plan": (C.c_int64, [u64p, sz, sz, sz, u64p, sz]),
        "ssa_debug_aggregates_many_coeffs": (i32, [vp, vp, u64p, sz, vp, vp, vp, sz, sz, vp]),
        "ssa_aggregates_many": (i32, [vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, u32, vp, vp, vp, u64p]),
        "ssa_aggregates_many_device": (i32, [vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, u32, vp, vp, vp, vp]),
        "ssa_debug_aggregates_fold_plan": (C.c_int64, [u64p, sz, u64p, sz]),
        "ssa_verify_aggregates_many_cached": (i32, [vp, vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, vp, vp]),
        "ssa_verify_aggregates_many_cached_device": (i32, [vp, vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, vp, vp]),
        "ssa_verify_aggregates_many_cached_wire": (i32, [vp, vp, vp, u64p, sz, vp, vp, vp, sz, sz, vp, vp]),
        "ssa_verify_aggregates_many_cached_wire_device": (i32, [vp, vp, vp, u64p, sz, vp, vp, vp, sz, sz, vp, vp]),
        "ssa_aggregator_create": (i32, [vp, sz, sz, u32, C.POINTER(vp)]),
        "ssa_aggregator_destroy": (None, [vp]),
        "ssa_aggregator_reset": (i32, [vp]),
        "ssa_aggregator_info": (i32, [vp, u64p]),
        "ssa_aggregator_push": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_aggregator_push_device": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]),
        "ssa_aggregator_finish": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_finish_device": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_push_cached": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u64p, vp]),
        "ssa_aggregator_push_cached_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u64p, vp]),
        "ssa_aggregator_push_keyed_cached": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u64p, vp]),
        "ssa_aggregator_push_keyed_cached_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, u64p, vp]),
        "ssa_aggregator_keys": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_keys_device": (i32, [vp, vp, sz, vp]),
        "ssa_debug_aggregator_bytes": (i32, [sz, sz, u32, u64p]),
        "ssa_debug_aggregator_bytes_ex": (i32, [sz, sz, u32, u64p]),
        "ssa_aggregator_admission": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_admission_device": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_leaves": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_leaves_device": (i32, [vp, vp, sz, vp]),
        "ssa_aggregator_leaves_select": (i32, [vp, vp, vp, sz, vp]),
        "ssa_aggregator_leaves_select_device": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_aggregator_index_sync": (i32, [vp, vp]),
        "ssa_aggregator_lookup": (i32, [vp, vp, vp, sz, vp, u64p]),
        "ssa_aggregator_lookup_device": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_aggregator_index_info": (i32, [vp, vp, u64p]),
        "ssa_debug_aggregator_plan": (i32, [C.c_uint64, C.c_uint64, C.c_uint64, u64p]),
        "ssa_aggregator_drop_front": (i32, [vp, vp, sz]),
        "ssa_aggregator_remove": (i32, [vp, vp, vp, sz, u64p]),
        "ssa_aggregator_remove_device": (i32, [vp, vp, vp, sz, u64p]),
        "ssa_debug_aggregator_remove_plan": (i32, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p]),
        "ssa_aggregator_finish_select": (i32, [vp, vp, vp, sz, vp, vp]),
        "ssa_aggregator_finish_select_device": (i32, [vp, vp, vp, sz, vp, vp, vp]),
        "ssa_aggregator_remove_indices": (i32, [vp, vp, vp, sz, u64p]),
        "ssa_aggregator_remove_indices_device": (i32, [vp, vp, vp, sz, u64p]),
        "ssa_aggverifier_create": (i32, [vp, sz, sz, u32, C.POINTER(vp)]),
        "ssa_aggverifier_destroy": (None, [vp]),
        "ssa_aggverifier_reset": (i32, [vp]),
        "ssa_aggverifier_info": (i32, [vp, u64p]),
        "ssa_aggverifier_push": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_aggverifier_push_device": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_aggverifier_finish": (i32, [vp, vp, vp, sz]),
        "ssa_aggverifier_finish_device": (i32, [vp, vp, vp, sz, vp]),
        "ssa_debug_aggverifier_record": (i32, [vp, vp, sz, vp]),
        "ssa_aggverifier_push_cached": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_aggverifier_push_cached_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_aggverifier_push_cached_wire": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_aggverifier_push_cached_wire_device": (i32, [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_debug_aggverifier_key_span": (sz, []),
        "ssa_aggverifier_push_mixed": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, sz]),
        "ssa_aggverifier_push_mixed_device": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, sz, vp]),
        "ssa_aggverifier_push_mixed_cached": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp]),
        "ssa_aggverifier_push_mixed_cached_device": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp,
                                                           vp]),
        "ssa_aggverifier_push_mixed_cached_wire": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, sz, sz, u32, vp]),
        "ssa_aggverifier_push_mixed_cached_wire_device": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, sz, sz, u32, vp,
                                                                vp]),
        "ssa_aggverifier_push_known": (i32, [vp, vp, vp, vp, sz]),
        "ssa_aggverifier_push_known_device": (i32, [vp, vp, vp, vp, sz, vp]),
        "ssa_debug_aggverifier_known_sum": (i32, [vp, vp, sz, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)      # AttributeError here == ABI symbol missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    # a library built from another revision of include/schnorr_sig_amd.h would still resolve every symbol and then
    # read its arguments shifted (round 2 inserted pk_inf into the batch entry points): refuse it at load
    got = lib.ssa_abi_version()
    if got != ABI_VERSION:
        raise ImportError("schnorr_sig_amd: %s has ABI version %d, this binding was written for %d -- rebuild "
                          "(python -c 'import __graft_entry__ as g; g.build(force=True)')" % (LIB_PATH, got, ABI_VERSION))
    return lib, list(sigs)


ABI_VERSION = 5        # SSA_ABI_VERSION of include/schnorr_sig_amd.h
MSM_PARTIAL_WORDS = 24
MSM_RECORD_MAGIC = 0x5353415245430004     # SSA_MSM_RECORD_MAGIC: word 23 of every shard record
_lib, ABI_SYMBOLS = _load()


def _check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, _lib.ssa_strerror(rc).decode(), rc))
    return rc


def _np_u8(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _addr(t):
    """the device address of a torch tensor; None for no tensor or an empty one"""
    return t.data_ptr() if t is not None and t.numel() else None


def _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride, no_msgs_ok=False):
    """(msg_stride, msg_len) of a device form over torch tensors: without an offset table and a given msg_len the rows
    of the 2-d d_msgs are the messages; msg_stride None: dense rows of msg_len bytes.  no_msgs_ok: the forms through a
    key cache, which take d_msgs None for a call without lanes."""
    if d_offsets is None and msg_len is None:
        msg_len = d_msgs.shape[1] if not (no_msgs_ok and d_msgs is None) and d_msgs.dim() == 2 else 0
    msg_len = msg_len or 0
    return msg_stride if msg_stride is not None else msg_len, msg_len


def pack_messages(messages):
    """list of bytes -> (concatenated uint8 array, uint64 offsets[n+1])."""
    off = np.zeros(len(messages) + 1, dtype=np.uint64)
    if messages:
        off[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    flat = np.frombuffer(b"".join(bytes(m) for m in messages) + b"\0", dtype=np.uint8).copy()
    return flat, off


def pack_aggregates(aggregates):
    """AggregateSignature objects or their bytes -> (counts uint64[k], the wire forms end to end as a uint8 array):
    aggregate j starts at byte 49 (n_0 + ... + n_(j-1)) + 32 j (ssa_verify_aggregates_many)"""
    raw = [bytes(a.bytes if isinstance(a, AggregateSignature) else a) for a in aggregates]
    for r in raw:
        if len(r) < 32 or (len(r) - 32) % 49:
            raise MalformedInput("an aggregate of n signatures is 49 n + 32 bytes")
    counts = np.array([(len(r) - 32) // 49 for r in raw], dtype=np.uint64)
    return counts, np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8).copy()


def split_aggregates(counts, wire):
    """the inverse of pack_aggregates: the wire forms end to end (49 N + 32 k bytes) -> the k aggregates as uint8 arrays
    (views of `wire`), aggregate j the 49 n_j + 32 bytes from byte 49 (n_0 + ... + n_(j-1)) + 32 j"""
    wire = _np_u8(wire).reshape(-1)
    out, lo = [], 0
    for n in counts:
        out.append(wire[lo:lo + 49 * int(n) + 32])
        lo += 49 * int(n) + 32
    if wire.size < lo:
        raise MalformedInput("k aggregates of N signatures are 49 N + 32 k bytes")
    return out


class Engine:
    """One ssa_ctx: a device, a stream, the comb table for G and the workspaces."""

    def __init__(self, device=0, params=None, gtab_bits=0, hbm_budget_bytes=0):
        """gtab_bits: window width of the comb for G (16 / 20 / 22 / 24; 0 = the widest whose table fits the budget);
        hbm_budget_bytes: device memory the speed-for-memory tables may take (0 = a tenth of what is free)."""
        self._ctx = C.c_void_p()
        blob = None
        if params is not None:
            blob = (C.c_uint8 * len(params)).from_buffer_copy(bytes(params))
        _check(_lib.ssa_ctx_create_ex(C.byref(self._ctx), int(device), blob, len(params) if params else 0,
                                      int(gtab_bits), int(hbm_budget_bytes)), "ssa_ctx_create_ex")
        self.device = int(device)

    def info(self):
        """what the context holds on the device (ssa_ctx_info)"""
        out = (C.c_uint64 * 8)()
        _check(_lib.ssa_ctx_info(self._ctx, out), "ssa_ctx_info")
        return {"gtab_bits": int(out[0]), "gtab_windows": int(out[1]), "gtab_bytes": int(out[2]),
                "workspace_bytes": int(out[3]), "lane_slice": int(out[4]), "msm_slice": int(out[5]),
                "hbm_budget_bytes": int(out[6]), "two_streams": bool(out[7])}

    def close(self):
        if self._ctx:
            _lib.ssa_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uses_default_params(self):
        """True when the context runs the builder-default (unpinned) Rescue constants and generator."""
        return bool(_check(_lib.ssa_ctx_uses_default_params(self._ctx), "ssa_ctx_uses_default_params"))

    @staticmethod
    def default_params():
        return C.string_at(_lib.ssa_default_params(), 2816)

    # ---- host-buffer entry points ------------------------------------------------------
    def _msg_args(self, msgs, offsets, n):
        if offsets is not None:
            m = _np_u8(msgs)
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            assert off.size == n + 1
            return m, off, 0, 0
        m = _np_u8(msgs)
        assert m.ndim == 2 and m.shape[0] == n, "dense messages must be an (n, len) array"
        return m, None, m.shape[1], m.shape[1]

    def _host_batch(self, sigs, pks, msgs, offsets, pk_inf, coeffs=None):
        """a batch in host memory as the verification entry points take it -> (n, the arguments from sigs to n in the
        order of the ABI, the pointer to the n x 32-byte coefficients or None, the arrays all of these point into: hold
        them until the call has returned).  An empty batch passes no signatures, keys or messages."""
        sigs, pks = _np_u8(sigs, 81), _np_u8(pks, 96)
        n = sigs.shape[0]
        if pks.shape[0] != n:
            raise MalformedInput("We should have the same number of signatures than public keys")
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        c = _np_u8(coeffs, 32) if coeffs is not None else None
        assert c is None or c.shape[0] == n
        batch = (_ptr(sigs) if n else None, _ptr(pks) if n else None, _ptr(inf), _ptr(m), _ptr(off), stride, mlen, n)
        return n, batch, _ptr(c), (sigs, pks, m, off, inf, c)

    @staticmethod
    def _dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n):
        """the arguments from pk_inf to n of a device form: 0 stands for no flags / no offset table, msg_stride None for
        dense rows of msg_len bytes"""
        return d_pk_inf or None, d_msgs, d_offsets or None, msg_stride if msg_stride is not None else msg_len, msg_len, n

    @staticmethod
    def _verify_flags(check_torsion, sig_flag_byte, mode=None):
        return (FLAG_CHECK_TORSION if check_torsion else 0) | _MODE_FLAGS[mode] | \
            (FLAG_SIG_FLAG_BYTE if sig_flag_byte else 0)

    def verify_many(self, sigs, pks, msgs, offsets=None, check_torsion=True, pk_inf=None, mode=None,
                    sig_flag_byte=False):
        """n x Signature::verify -> (status uint8[n], n_fail).  mode: None/"auto" (wave-per-signature
        kernel for small batches, lane-per-signature kernels for large ones), "lane" or "coop".
        sig_flag_byte: honour byte 48 of the signature as verify_batch does (src/batch.rs:104)."""
        n, batch, _, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        _check(_lib.ssa_verify_many(self._ctx, *batch, self._verify_flags(check_torsion, sig_flag_byte, mode),
                                    _ptr(status) if n else None, C.byref(nfail)), "ssa_verify_many")
        return status, int(nfail.value)

    def verify_many_dedup(self, sigs, pks, msgs, offsets=None, check_torsion=True, pk_inf=None, mode=None,
                          sig_flag_byte=False):
        """verify_many with each distinct public key of a slice checked once on the GPU ->
        (status uint8[n], n_fail, stats uint64[4]); status and n_fail are those of verify_many.  stats: distinct keys
        summed over slices, slices on the keyed route, slices that fell back, lanes that hit the probe bound."""
        n, batch, _, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        stats = np.zeros(4, dtype=np.uint64)
        _check(_lib.ssa_verify_many_dedup(self._ctx, *batch, self._verify_flags(check_torsion, sig_flag_byte, mode),
                                          _ptr(status) if n else None, C.byref(nfail), stats.ctypes.data),
               "ssa_verify_many_dedup")
        return status, int(nfail.value), stats

    def verify_many_dedup_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_status, d_nfail, msg_stride=None,
                                 d_offsets=0, d_pk_inf=0, check_torsion=False, mode=None, sig_flag_byte=False):
        """device form of verify_many_dedup (synchronises the stream once per slice to read the number of distinct keys);
        returns the statistics (uint64[4], host)"""
        stats = np.zeros(4, dtype=np.uint64)
        _check(_lib.ssa_verify_many_dedup_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            self._verify_flags(check_torsion, sig_flag_byte, mode), d_status, d_nfail or None, stats.ctypes.data),
            "ssa_verify_many_dedup_device")
        return stats

    def debug_dedup_device(self, d_pks, n, d_key_idx=0, d_pk_inf=0):
        """tests: the key dedup alone over one slice of device keys -> (distinct keys, lanes at the probe bound);
        d_key_idx (optional, device, n x uint32) receives each lane's key index"""
        out = np.zeros(2, dtype=np.uint64)
        _check(_lib.ssa_debug_dedup_device(self._ctx, d_pks, d_pk_inf or None, n, d_key_idx or None, out.ctypes.data),
               "ssa_debug_dedup_device")
        return int(out[0]), int(out[1])

    def debug_dedup_config(self, max_distinct_ratio=-1.0, probe_bound=0):
        """tests: the policy of verify_many_dedup on this engine -- keyed route when u < max_distinct_ratio * lanes
        (0 forces the fallback, above 1 the keyed route, negative: the measured defaults), probes per lane (0: the
        default)"""
        _check(_lib.ssa_debug_dedup_config(self._ctx, float(max_distinct_ratio), int(probe_bound)),
               "ssa_debug_dedup_config")

    def verify_batch_status(self, sigs, pks, msgs, offsets=None, check_torsion=False, pk_inf=None):
        n, batch, _, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf)
        return _check(_lib.ssa_verify_batch(self._ctx, *batch, FLAG_CHECK_TORSION if check_torsion else 0),
                      "ssa_verify_batch")

    def verify_batch_msm(self, sigs, pks, msgs, offsets=None, coeffs=None, pk_inf=None):
        """verify_batch as the reference runs it (random linear combination + MSM); one status."""
        n, batch, c, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf, coeffs)
        return _check(_lib.ssa_verify_batch_msm(self._ctx, *batch, c), "ssa_verify_batch_msm")

    def verify_batch_msm_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_verdict,
                                msg_stride=None, d_offsets=0, d_pk_inf=0):
        _check(_lib.ssa_verify_batch_msm_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n), d_coeffs,
            coeff_bytes, d_verdict), "ssa_verify_batch_msm_device")

    def verify_batch_screened(self, sigs, pks, msgs, offsets=None, coeffs=None, pk_inf=None):
        """verify_batch semantics per signature at about the price of the MSM verdict -> (status uint8[n], n_fail).
        Segments of the batch are screened by the MSM; only lanes of failing segments run the per-lane check
        (include/schnorr_sig_amd.h).  coeffs: n x 32-byte scalars, or None (drawn on the device)."""
        n, batch, c, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf, coeffs)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        _check(_lib.ssa_verify_batch_screened(self._ctx, *batch, c, _ptr(status) if n else None, C.byref(nfail)),
               "ssa_verify_batch_screened")
        return status, int(nfail.value)

    def verify_batch_screened_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_status, d_nfail,
                                     msg_stride=None, d_offsets=0, d_pk_inf=0):
        """device form (synchronises the stream once per slice to read the segment verdicts)"""
        _check(_lib.ssa_verify_batch_screened_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            d_coeffs or None, coeff_bytes, d_status, d_nfail or None), "ssa_verify_batch_screened_device")

    def verify_many_screened(self, sigs, pks, msgs, offsets=None, check_torsion=True, pk_inf=None, sig_flag_byte=False,
                             coeffs=None):
        """the status vector of verify_many at about the price of one MSM -> (status uint8[n],
        n_fail, stats uint64[8]).  Each distinct key of a slice is checked once, the segments of the slice are screened
        by the MSM, and only the lanes of failing segments and the lanes that could not be screened run the exact keyed
        kernel.  check_torsion alone is Signature::verify; sig_flag_byte alone is verify_batch_screened.  coeffs: n x
        32-byte scalars, or None (drawn on the device).  stats: distinct keys, segments screened, segments that failed,
        lanes re-checked, lanes that could not be screened, slices screened, slices run entirely by the exact kernel,
        lanes at the dedup probe bound."""
        n, batch, c, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf, coeffs)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        stats = np.zeros(8, dtype=np.uint64)
        _check(_lib.ssa_verify_many_screened(self._ctx, *batch, self._verify_flags(check_torsion, sig_flag_byte), c,
                                             _ptr(status) if n else None, C.byref(nfail), stats.ctypes.data),
               "ssa_verify_many_screened")
        return status, int(nfail.value), stats

    def verify_many_screened_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_status, d_nfail,
                                    msg_stride=None, d_offsets=0, d_pk_inf=0, check_torsion=True, sig_flag_byte=False):
        """device form of verify_many_screened (synchronises the stream twice per slice: for the number of distinct
        keys, and for the segment verdicts with the length of the re-check list); returns the statistics (uint64[8],
        host)"""
        stats = np.zeros(8, dtype=np.uint64)
        _check(_lib.ssa_verify_many_screened_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            self._verify_flags(check_torsion, sig_flag_byte), d_coeffs or None, coeff_bytes, d_status, d_nfail or None,
            stats.ctypes.data), "ssa_verify_many_screened_device")
        return stats

    def keycache_create(self, capacity, wire=False, evict="clear"):
        """a key cache of `capacity` keys on this engine's device: all of its device memory, about
        4.2 KB per key, is allocated here.  wire=True (SSA_KEYCACHE_WIRE): a key is identified by
        its 49 compressed bytes as received; such a cache serves verify_keyed_many_cached and (with dense 49-byte keys)
        verify_aggregates_cached, and no other call.
        evict="recent" (KeyCache.set_eviction): a full cache keeps the keys used most recently
        instead of clearing itself."""
        if evict not in KEYCACHE_EVICT:
            raise ValueError("evict must be one of %s" % sorted(KEYCACHE_EVICT))
        h = C.c_void_p()
        _check(_lib.ssa_keycache_create_ex(self._ctx, int(capacity), KEYCACHE_WIRE if wire else 0, C.byref(h)),
               "ssa_keycache_create_ex")
        cache = KeyCache(self, h, wire=wire)
        if evict != "clear":
            try:
                cache.set_eviction(evict)
            except Exception:
                cache.close()
                raise
        return cache

    def aggregator(self, capacity, block_lanes=0, hold_keys=False, hold_admission=False, index=False):
        """a streaming aggregator of `capacity` lanes on this engine's device: push signatures
        as they arrive, finish at block time.  All of its device memory, about 113 bytes per lane, is allocated here.
        block_lanes: 0 (512) or a power of two from 2 to 512.
        hold_keys=True (SSA_AGGR_HOLD_KEYS49): the object also holds every admitted lane's 49-byte
        wire key (49 more bytes per lane) for Aggregator.keys(); it then takes push_keyed alone.
        hold_admission=True (SSA_AGGR_HOLD_ADMISSION): the object also records the class of the
        push that admitted each lane (one more byte per lane) for Aggregator.admission() and for
        AggregateVerifier.push_mixed(cache=, require=).
        index=True (SSA_AGGR_HOLD_INDEX): the object also holds a leaf index (32 bytes per lane
        of the capacity and more: 8 bytes per slot, at least four slots per lane) for Aggregator.lookup(): which place
        holds this id?"""
        h = C.c_void_p()
        _check(_lib.ssa_aggregator_create(self._ctx, int(capacity), int(block_lanes),
                                          _aggr_flags(hold_keys, hold_admission, index), C.byref(h)), "ssa_aggregator_create")
        return Aggregator(self, h, hold_keys=hold_keys, hold_admission=hold_admission, index=index)

    def aggregate_verifier(self, capacity, block_lanes=0):
        """a streaming aggregate verifier of `capacity` lanes on this engine's device: push the
        R's, keys and messages of a block body as they arrive, finish with e_agg.  All of its device memory, about 259
        bytes per lane, is allocated here.  block_lanes: 0 (512) or a power of two from 2 to 512."""
        h = C.c_void_p()
        _check(_lib.ssa_aggverifier_create(self._ctx, int(capacity), int(block_lanes), 0, C.byref(h)),
               "ssa_aggverifier_create")
        return AggregateVerifier(self, h)

    def verify_keyed_many_cached(self, cache, keyed, msgs, offsets=None, check_torsion=True, sig_flag_byte=False,
                                 coeffs=None):
        """verify_many_cached on 130-byte KeyedSignature records pk(49) || sig(81) through a cache made with wire=True
         -> (status uint8[n], n_fail, stats uint64[12]).  A key that was seen before -- one that
        does not decode included -- is neither decompressed nor checked again.  With the same coeffs the status vector is
        byte for byte verify_many_screened on the unpacked records, in every state of the cache.  stats as
        verify_many_cached; [0], [8] and [9] count distinct 49-byte strings."""
        kd = _np_u8(keyed, 130)
        n = kd.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        c = None
        if coeffs is not None:
            c = _np_u8(coeffs, 32)
            if c.shape[0] != n:
                raise ValueError("coeffs needs one 32-byte scalar per record")
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64)
        _check(_lib.ssa_verify_keyed_many_cached(self._ctx, cache.handle, _ptr(kd), _ptr(m), _ptr(off), stride, mlen, n,
                                                 self._verify_flags(check_torsion, sig_flag_byte), _ptr(c),
                                                 _ptr(status) if n else None, C.byref(nfail), stats.ctypes.data),
               "ssa_verify_keyed_many_cached")
        return status, int(nfail.value), stats

    def verify_keyed_many_cached_device(self, cache, d_keyed, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_status, d_nfail,
                                        msg_stride=None, d_offsets=0, check_torsion=True, sig_flag_byte=False):
        """device form of verify_keyed_many_cached (two synchronisations per slice; the slices run in order on the
        engine's stream); returns the statistics (uint64[12], host)"""
        stats = np.zeros(12, dtype=np.uint64)
        _check(_lib.ssa_verify_keyed_many_cached_device(
            self._ctx, cache.handle, d_keyed, *self._dev_batch(0, d_msgs, d_offsets, msg_stride, msg_len, n)[1:],
            self._verify_flags(check_torsion, sig_flag_byte), d_coeffs or None, coeff_bytes, d_status, d_nfail or None,
            stats.ctypes.data), "ssa_verify_keyed_many_cached_device")
        return stats

    def verify_keyed_many_device(self, d_keyed, d_msgs, n, msg_len, d_status, d_nfail, msg_stride=None, d_offsets=0,
                                 check_torsion=True):
        """device form of verify_keyed_many (enqueued on the engine's stream)"""
        _check(_lib.ssa_verify_keyed_many_device(
            self._ctx, d_keyed, *self._dev_batch(0, d_msgs, d_offsets, msg_stride, msg_len, n)[1:],
            FLAG_CHECK_TORSION if check_torsion else 0, d_status, d_nfail or None), "ssa_verify_keyed_many_device")

    def verify_many_cached(self, cache, sigs, pks, msgs, offsets=None, check_torsion=True, pk_inf=None,
                           sig_flag_byte=False, coeffs=None):
        """verify_many_screened with the per-key check behind a key cache -> (status uint8[n],
        n_fail, stats uint64[12]).  The status vector is byte for byte the one verify_many_screened returns with the
        same coeffs, in every state of the cache.  stats[0..7] as verify_many_screened (rows that could not be published
        are added to [7]); [8] distinct keys found in the cache, [9] keys checked and inserted, [10] automatic clears,
        [11] slices that bypassed the cache."""
        n, batch, c, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf, coeffs)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64)
        _check(_lib.ssa_verify_many_cached(self._ctx, cache.handle, *batch,
                                           self._verify_flags(check_torsion, sig_flag_byte), c,
                                           _ptr(status) if n else None, C.byref(nfail), stats.ctypes.data),
               "ssa_verify_many_cached")
        return status, int(nfail.value), stats

    def verify_many_cached_device(self, cache, d_sigs, d_pks, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_status, d_nfail,
                                  msg_stride=None, d_offsets=0, d_pk_inf=0, check_torsion=True, sig_flag_byte=False):
        """device form of verify_many_cached (two synchronisations per slice, as verify_many_screened_device; the slices
        run in order on the engine's stream); returns the statistics (uint64[12], host)"""
        stats = np.zeros(12, dtype=np.uint64)
        _check(_lib.ssa_verify_many_cached_device(
            self._ctx, cache.handle, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            self._verify_flags(check_torsion, sig_flag_byte), d_coeffs or None, coeff_bytes, d_status, d_nfail or None,
            stats.ctypes.data), "ssa_verify_many_cached_device")
        return stats

    def debug_screen_segments(self, k):
        """tests: k segments per slice in the screened form on this engine (0 = automatic)"""
        _check(_lib.ssa_debug_screen_segments(self._ctx, int(k)), "ssa_debug_screen_segments")

    # ---- MSM-form verdict across processes: per-shard records + combination (include/schnorr_sig_amd.h) ----
    def verify_batch_msm_partial_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_coeffs, coeff_bytes, d_partial24,
                                        msg_stride=None, d_offsets=0, d_pk_inf=0):
        """this rank's shard -> one 24-word record at device address d_partial24 (enqueued on the stream)"""
        _check(_lib.ssa_verify_batch_msm_partial_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            d_coeffs or None, coeff_bytes, d_partial24), "ssa_verify_batch_msm_partial_device")

    def verify_batch_msm_partial(self, sigs, pks, msgs, offsets=None, coeffs=None, pk_inf=None):
        """host buffers -> the shard's record as uint64[24]"""
        n, batch, c, keep = self._host_batch(sigs, pks, msgs, offsets, pk_inf, coeffs)
        out = np.zeros(MSM_PARTIAL_WORDS, dtype=np.uint64)
        _check(_lib.ssa_verify_batch_msm_partial(self._ctx, *batch, c, _ptr(out)), "ssa_verify_batch_msm_partial")
        return out

    def msm_combine_device(self, d_parts24, k, d_verdict):
        _check(_lib.ssa_msm_combine_device(self._ctx, d_parts24, k, d_verdict), "ssa_msm_combine_device")

    def msm_combine(self, parts):
        """uint64[k, 24] records (host) -> status of the whole batch"""
        parts = np.ascontiguousarray(parts, dtype=np.uint64).reshape(-1, MSM_PARTIAL_WORDS)
        return _check(_lib.ssa_msm_combine(self._ctx, _ptr(parts), parts.shape[0]), "ssa_msm_combine")

    # ---- half-aggregation (include/schnorr_sig_amd.h) ----
    def _agg_batch(self, lead, width, pks, msgs, offsets, pk_inf):
        """(n, the arguments from the leading array to n, the arrays they point into): `lead` holds `width` bytes per
        lane, plus 32 bytes of e_agg when it is an aggregate (width 49 and a length that says so)"""
        pks = _np_u8(pks, 96)
        n = pks.shape[0]
        lead = _np_u8(lead).reshape(-1)
        if lead.size not in (width * n, width * n + 32 if width == 49 else -1):
            raise MalformedInput("We should have the same number of signatures than public keys")
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        return n, (_ptr(lead), _ptr(pks) if n else None, _ptr(inf), _ptr(m), _ptr(off), stride, mlen, n), (lead, pks, m, off, inf)

    def aggregate(self, sigs, pks, msgs, offsets=None, pk_inf=None, check=False):
        """n signatures -> (status, aggregate uint8[49 n + 32], per-lane status uint8[n], n_fail): the n R's and
        e_agg = sum a_i e_i mod q.  check: screen the signatures first (SSA_AGG_CHECK).  A nonzero status (the smallest
        of the lanes') comes with an all-zero aggregate."""
        n, batch, keep = self._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        st = _check(_lib.ssa_aggregate_many(self._ctx, *batch, AGG_CHECK if check else 0, _ptr(agg),
                                            _ptr(status) if n else None, C.byref(nfail)), "ssa_aggregate_many")
        return st, agg, status, int(nfail.value)

    def aggregate_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_agg, d_status=0, d_nfail=0, msg_stride=None,
                         d_offsets=0, d_pk_inf=0, check=False):
        """device form (synchronises the stream: the status is read from the device) -> status"""
        return _check(_lib.ssa_aggregate_many_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            AGG_CHECK if check else 0, d_agg, d_status or None, d_nfail or None), "ssa_aggregate_many_device")

    def verify_aggregate(self, agg, pks, msgs, offsets=None, pk_inf=None):
        """an aggregate (49 n + 32 bytes), the keys and the messages in the aggregator's order -> status"""
        n, batch, keep = self._agg_batch(agg, 49, pks, msgs, offsets, pk_inf)
        if keep[0].size != 49 * n + 32:
            raise MalformedInput("an aggregate of n signatures is 49 n + 32 bytes")
        return _check(_lib.ssa_verify_aggregate(self._ctx, *batch), "ssa_verify_aggregate")

    def verify_aggregate_device(self, d_agg, d_pks, d_msgs, n, msg_len, d_verdict, msg_stride=None, d_offsets=0,
                                d_pk_inf=0):
        """device form: only enqueues; the status lands in the uint32 at d_verdict"""
        _check(_lib.ssa_verify_aggregate_device(
            self._ctx, d_agg, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n), d_verdict),
            "ssa_verify_aggregate_device")

    # ---- sharded half-aggregation (include/schnorr_sig_amd.h) ----
    def aggregate_sliced(self, sigs, pks, msgs, offsets=None, pk_inf=None, check=False):
        """aggregate() for any n <= SSA_MAX_BATCH: slice after slice of this context, the same bytes"""
        n, batch, keep = self._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        st = _check(_lib.ssa_aggregate_many_sliced(self._ctx, *batch, AGG_CHECK if check else 0, _ptr(agg),
                                                   _ptr(status) if n else None, C.byref(nfail)),
                    "ssa_aggregate_many_sliced")
        return st, agg, status, int(nfail.value)

    def aggregate_sliced_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_agg, d_status=0, d_nfail=0, msg_stride=None,
                                d_offsets=0, d_pk_inf=0, check=False):
        """device form of aggregate_sliced (synchronises the stream, as aggregate_device does) -> status"""
        return _check(_lib.ssa_aggregate_many_sliced_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            AGG_CHECK if check else 0, d_agg, d_status or None, d_nfail or None), "ssa_aggregate_many_sliced_device")

    def verify_aggregate_sliced(self, agg, pks, msgs, offsets=None, pk_inf=None):
        """verify_aggregate() for any n <= SSA_MAX_BATCH -> status"""
        n, batch, keep = self._agg_batch(agg, 49, pks, msgs, offsets, pk_inf)
        if keep[0].size != 49 * n + 32:
            raise MalformedInput("an aggregate of n signatures is 49 n + 32 bytes")
        return _check(_lib.ssa_verify_aggregate_sliced(self._ctx, *batch), "ssa_verify_aggregate_sliced")

    def verify_aggregate_sliced_device(self, d_agg, d_pks, d_msgs, n, msg_len, d_verdict, msg_stride=None, d_offsets=0,
                                       d_pk_inf=0):
        """device form: only enqueues; the status lands in the uint32 at d_verdict"""
        _check(_lib.ssa_verify_aggregate_sliced_device(
            self._ctx, d_agg, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n), d_verdict),
            "ssa_verify_aggregate_sliced_device")

    # The shard primitives: device addresses, everything only enqueued on the engine's stream.  A shard is n_s
    # consecutive lanes of an aggregate whose first, lane0, stands on a multiple of block_lanes.
    def aggregate_shard_tops_device(self, d_lanes, lane_stride, d_pks, d_msgs, n_s, msg_len, block_lanes, d_tops, d_h=0,
                                    msg_stride=None, d_offsets=0):
        """n_s signatures (lane_stride 81) or R's (49) -> ceil(n_s / block_lanes) x 32 bytes of tops at d_tops; d_h: the
        n_s x 32 bytes of challenge scalars the validator's shard call takes"""
        _check(_lib.ssa_aggregate_shard_tops_device(
            self._ctx, d_lanes, lane_stride, d_pks, d_msgs, d_offsets or None,
            msg_stride if msg_stride is not None else msg_len, msg_len, n_s, block_lanes, d_tops, d_h or None),
            "ssa_aggregate_shard_tops_device")

    def aggregate_root_device(self, d_tops, n_tops, n, d_root, block_lanes=0):
        """the tops of all shards in lane order and the total n -> the 32-byte root at d_root"""
        _check(_lib.ssa_aggregate_root_device(self._ctx, d_tops, n_tops, n, block_lanes, d_root),
               "ssa_aggregate_root_device")

    def aggregate_shard_fold_device(self, d_sigs, d_pks, n_s, lane0, d_root, d_e, d_rs, d_status=0, d_nfail=0, d_pk_inf=0):
        """producer: the shard's sum a_i e_i mod q (32 bytes at d_e) and its R's (49 n_s bytes at d_rs); d_status: the
        checks of aggregate() without check=True, one byte per lane"""
        _check(_lib.ssa_aggregate_shard_fold_device(self._ctx, d_sigs, d_pks or None, d_pk_inf or None, n_s, lane0, d_root,
                                                    d_e, d_rs or None, d_status or None, d_nfail or None),
               "ssa_aggregate_shard_fold_device")

    def verify_aggregate_shard_device(self, d_rs49, d_pks, d_msgs, n_s, msg_len, d_h, lane0, d_root, d_record24,
                                      msg_stride=None, d_offsets=0, d_pk_inf=0):
        """validator: the shard's R's, keys, messages and saved challenge scalars -> one 24-word record at d_record24"""
        _check(_lib.ssa_verify_aggregate_shard_device(
            self._ctx, d_rs49 or None, d_pks or None, d_pk_inf or None, d_msgs, d_offsets or None,
            msg_stride if msg_stride is not None else msg_len, msg_len, d_h or None, n_s, lane0, d_root, d_record24),
            "ssa_verify_aggregate_shard_device")

    def aggregate_combine_device(self, d_partials32, k, d_e_agg):
        """k partial scalars (32 bytes each) -> e_agg at d_e_agg"""
        _check(_lib.ssa_aggregate_combine_device(self._ctx, d_partials32, k, d_e_agg), "ssa_aggregate_combine_device")

    def verify_aggregate_combine_device(self, d_records24, k, d_e_agg, n, d_verdict):
        """k records, e_agg and the total n -> the status in the uint32 at d_verdict; fails closed (MALFORMED) on a
        record that is not one"""
        _check(_lib.ssa_verify_aggregate_combine_device(self._ctx, d_records24 or None, k, d_e_agg, n, d_verdict),
               "ssa_verify_aggregate_combine_device")

    def aggregate_shard_coeffs(self, root32, n_s, lane0):
        """tests: the coefficients of lanes [lane0, lane0 + n_s) of an aggregate with this root -> uint8[n_s, 16]"""
        root = _np_u8(root32).reshape(32)
        out = np.zeros((n_s, 16), dtype=np.uint8)
        _check(_lib.ssa_debug_aggregate_shard_coeffs(self._ctx, _ptr(root), n_s, lane0, _ptr(out) if n_s else None),
               "ssa_debug_aggregate_shard_coeffs")
        return out

    def aggregate_coeffs(self, rs49, pks, msgs, offsets=None, pk_inf=None):
        """tests: the transcript's coefficients a_i of n R's (n x 49 bytes), keys and messages -> uint8[n, 16]"""
        n, batch, keep = self._agg_batch(rs49, 49, pks, msgs, offsets, pk_inf)
        if keep[0].size != 49 * n:
            raise MalformedInput("n R's are 49 n bytes")
        out = np.zeros((n, 16), dtype=np.uint8)
        _check(_lib.ssa_debug_aggregate_coeffs(self._ctx, *batch, _ptr(out) if n else None), "ssa_debug_aggregate_coeffs")
        return out

    # ---- filtering half-aggregation (include/schnorr_sig_amd.h) ----
    def aggregate_valid(self, sigs, pks, msgs, offsets=None, pk_inf=None):
        """n signatures -> (aggregate uint8[49 |K| + 32] of the lanes that verify, their indices uint32[|K|] ascending,
        per-lane status uint8[n] as verify_batch_screened gives it).  The aggregate is what aggregate() returns for
        those lanes handed in alone; with none kept it is the 32 zero bytes of the empty aggregate."""
        n, batch, keep = self._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        kept = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        status = np.full(n, 255, dtype=np.uint8)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregate_valid_many(self._ctx, *batch, _ptr(agg), _ptr(kept), C.byref(n_kept),
                                             _ptr(status) if n else None), "ssa_aggregate_valid_many")
        m = int(n_kept.value)
        return agg[:49 * m + 32].copy(), kept[:m].copy(), status

    def aggregate_valid_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_agg, d_kept, d_status=0, msg_stride=None,
                               d_offsets=0, d_pk_inf=0):
        """device form (synchronises the stream twice: inside the screen and for the number of kept lanes) -> that
        number; the aggregate of the kept lanes lands at d_agg (capacity 49 n + 32 bytes, zero behind it), their indices
        at d_kept (capacity n uint32, zero behind them), the statuses at d_status if it is given"""
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregate_valid_many_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            d_agg, d_kept, C.byref(n_kept), d_status or None), "ssa_aggregate_valid_many_device")
        return int(n_kept.value)

    # ---- filtering half-aggregation through a key cache (include/schnorr_sig_amd.h) ----
    def aggregate_valid_cached(self, cache, sigs, pks, msgs, offsets=None, pk_inf=None):
        """aggregate_valid under the statuses of verify_many_cached(check_torsion=True, sig_flag_byte=True): a lane whose
        key lies outside the prime-order subgroup is dropped (status INVALID_PUBLIC_KEY) -> (aggregate uint8[49 |K| + 32],
        kept uint32[|K|], status uint8[n], the kept keys uint8[|K|, 96], their pk_inf uint8[|K|], stats uint64[12] as
        verify_many_cached).  Aggregate and kept keys are what verify_aggregates_cached takes on the same cache."""
        if cache.wire:
            raise ValueError("an affine batch takes an affine key cache (records: aggregate_valid_keyed_cached)")
        n, batch, keep = self._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        kept = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        status = np.full(n, 255, dtype=np.uint8)
        pks_out = np.full((max(n, 1), 96), 255, dtype=np.uint8)
        inf_out = np.full(max(n, 1), 255, dtype=np.uint8)
        stats = np.zeros(12, dtype=np.uint64)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregate_valid_many_cached(self._ctx, cache.handle, *batch, _ptr(agg), _ptr(kept), C.byref(n_kept),
                                                    _ptr(status) if n else None, _ptr(pks_out), _ptr(inf_out),
                                                    stats.ctypes.data), "ssa_aggregate_valid_many_cached")
        m = int(n_kept.value)
        return agg[:49 * m + 32].copy(), kept[:m].copy(), status, pks_out[:m].copy(), inf_out[:m].copy(), stats

    def aggregate_valid_keyed_cached(self, cache, keyed, msgs, offsets=None):
        """aggregate_valid_cached on 130-byte KeyedSignature records pk(49) || sig(81) through a cache made with
        wire=True -> (aggregate, kept uint32[|K|], status uint8[n] as verify_keyed_many_cached gives it, the kept keys
        uint8[|K|, 49], stats uint64[12])"""
        if not cache.wire:
            raise ValueError("records take a key cache made with wire=True")
        kd = _np_u8(keyed, 130)
        n = kd.shape[0]
        m_, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        kept = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        status = np.full(n, 255, dtype=np.uint8)
        keys_out = np.full((max(n, 1), 49), 255, dtype=np.uint8)
        stats = np.zeros(12, dtype=np.uint64)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregate_valid_keyed_many_cached(
            self._ctx, cache.handle, _ptr(kd) if n else None, _ptr(m_), _ptr(off), stride, mlen, n, _ptr(agg), _ptr(kept),
            C.byref(n_kept), _ptr(status) if n else None, _ptr(keys_out), stats.ctypes.data),
            "ssa_aggregate_valid_keyed_many_cached")
        m = int(n_kept.value)
        return agg[:49 * m + 32].copy(), kept[:m].copy(), status, keys_out[:m].copy(), stats

    def aggregate_valid_cached_device(self, cache, d_sigs, d_pks, d_msgs, n, msg_len, d_agg, d_kept, d_status=0, d_pks_out=0,
                                      d_pk_inf_out=0, msg_stride=None, d_offsets=0, d_pk_inf=0, want_stats=True):
        """device form of aggregate_valid_cached (device addresses; the synchronisations of verify_many_cached_device
        and one for the number of kept lanes) -> (that number, stats uint64[12] or None).  Capacities: d_agg 49 n + 32
        bytes, d_kept n uint32, d_pks_out 96 n bytes, d_pk_inf_out n bytes; all zero behind the kept lanes."""
        n_kept = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggregate_valid_many_cached_device(
            self._ctx, cache.handle, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            d_agg, d_kept, C.byref(n_kept), d_status or None, d_pks_out or None, d_pk_inf_out or None,
            stats.ctypes.data if want_stats else None), "ssa_aggregate_valid_many_cached_device")
        return int(n_kept.value), stats

    def aggregate_valid_keyed_cached_device(self, cache, d_keyed, d_msgs, n, msg_len, d_agg, d_kept, d_status=0,
                                            d_keys49_out=0, msg_stride=None, d_offsets=0, want_stats=True):
        """device form of aggregate_valid_keyed_cached -> (the number of kept lanes, stats uint64[12] or None);
        d_keys49_out: capacity 49 n bytes"""
        n_kept = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggregate_valid_keyed_many_cached_device(
            self._ctx, cache.handle, d_keyed, *self._dev_batch(0, d_msgs, d_offsets, msg_stride, msg_len, n)[1:],
            d_agg, d_kept, C.byref(n_kept), d_status or None, d_keys49_out or None,
            stats.ctypes.data if want_stats else None), "ssa_aggregate_valid_keyed_many_cached_device")
        return int(n_kept.value), stats

    def debug_aggregate_keep(self, status):
        """tests: the compaction alone -> (the indices of the zero bytes of `status`, ascending, as the device lists
        them; the whole uint32[n] output, zero behind the list)"""
        status = _np_u8(status).reshape(-1)
        n = status.size
        kept = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_debug_aggregate_keep(self._ctx, _ptr(status) if n else None, n, _ptr(kept) if n else None,
                                             C.byref(n_kept)), "ssa_debug_aggregate_keep")
        return kept[:int(n_kept.value)], kept[:n]

    # ---- many aggregates in one call (include/schnorr_sig_amd.h) ----
    def _aggs_batch(self, aggregates, pks, msgs, offsets, pk_inf):
        """(counts uint64[k], the wire bytes end to end, keys, messages, offsets, stride, length, flags) of a list of
        AggregateSignature objects or byte strings; the keys and messages of all lanes follow in the same order"""
        counts, wire = pack_aggregates(aggregates)
        n = int(counts.sum())
        pks = _np_u8(pks, 96)
        if pks.shape[0] != n:
            raise MalformedInput("We should have the same number of signatures than public keys")
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        return counts, wire, pks, m, off, stride, mlen, inf

    def verify_aggregates(self, aggregates, pks, msgs, pk_inf=None, offsets=None):
        """k aggregates (AggregateSignature objects or their bytes), the keys and messages of all their lanes in order
        -> uint32[k]: for each aggregate the status verify_aggregate gives it alone"""
        counts, wire, pks, m, off, stride, mlen, inf = self._aggs_batch(aggregates, pks, msgs, offsets, pk_inf)
        k = counts.size
        out = np.full(k, 255, dtype=np.uint32)
        _check(_lib.ssa_verify_aggregates_many(
            self._ctx, _ptr(wire) if k else None, counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k,
            _ptr(pks) if pks.shape[0] else None, _ptr(inf), _ptr(m), _ptr(off), stride, mlen, _ptr(out) if k else None),
            "ssa_verify_aggregates_many")
        return out

    def verify_aggregates_device(self, d_aggs, counts, d_pks, d_msgs, d_verdicts=None, d_pk_inf=None, d_offsets=None,
                                 msg_len=None, msg_stride=None):
        """device form over torch tensors on this engine's device: d_aggs the wire bytes end to end, counts a HOST
        sequence, d_msgs an (N, len) uint8 tensor (or flat bytes with a uint64-valued d_offsets and msg_len left None).
        Only enqueues; the statuses land in d_verdicts (int32[k], allocated when None), which is returned."""
        import torch
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        k = counts.size
        if d_verdicts is None:
            d_verdicts = torch.empty(max(k, 1), dtype=torch.int32, device=d_aggs.device)[:k]
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
        _check(_lib.ssa_verify_aggregates_many_device(
            self._ctx, _addr(d_aggs), counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k, _addr(d_pks),
            _addr(d_pk_inf), _addr(d_msgs), _addr(d_offsets), stride, mlen, _addr(d_verdicts)),
            "ssa_verify_aggregates_many_device")
        return d_verdicts

    # ---- many aggregates produced in one call (include/schnorr_sig_amd.h) ----
    def aggregates_wire(self, batches, check=False, counts=None, pk_inf=None, offsets=None):
        """k batches of signatures -> (counts uint64[k]; wire uint8[49 N + 32 k], the aggregates end to end as the call
        wrote them and as verify_aggregates reads them, a refused one all zero; results uint32[k]; per-lane status
        uint8[N]; n_fail).  batches: a list of (sigs, pks, msgs) or (sigs, pks, msgs, pk_inf) batches, msgs an (n, len)
        array or a list of byte strings; or, with counts, the flat (sigs, pks, msgs) of all N lanes in order, with pk_inf
        and offsets as verify_aggregates takes them.  results[j]: OK, MALFORMED or, with check, the smallest nonzero
        status of batch j's lanes."""
        if counts is None:
            counts = np.array([_np_u8(b[1], 96).shape[0] for b in batches], dtype=np.uint64)
            n = int(counts.sum())
            sigs = np.concatenate([_np_u8(b[0], 81) for b in batches] + [np.zeros((0, 81), np.uint8)])
            pks = np.concatenate([_np_u8(b[1], 96) for b in batches] + [np.zeros((0, 96), np.uint8)])
            if any(len(b) > 3 and b[3] is not None for b in batches):
                pk_inf = np.concatenate([_np_u8(b[3]).reshape(-1) if len(b) > 3 and b[3] is not None
                                         else np.zeros(int(c), np.uint8) for b, c in zip(batches, counts)])
            rows = [b[2] for b, c in zip(batches, counts) if c]
            if rows and all(isinstance(r, np.ndarray) and r.ndim == 2 and r.shape[1] == rows[0].shape[1] for r in rows):
                msgs = np.concatenate(rows)
            else:
                msgs, offsets = pack_messages([bytes(m) for r in rows for m in r])
        else:
            sigs, pks, msgs = batches
            counts = np.ascontiguousarray(counts, dtype=np.uint64)
            n = int(counts.sum())
            sigs, pks = _np_u8(sigs, 81), _np_u8(pks, 96)
        if sigs.shape[0] != n or pks.shape[0] != n:
            raise MalformedInput("We should have the same number of signatures than public keys")
        k = counts.size
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        wire = np.full(49 * n + 32 * k + 1, 255, dtype=np.uint8)
        results = np.full(k, 255, dtype=np.uint32)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        _check(_lib.ssa_aggregates_many(
            self._ctx, _ptr(sigs) if n else None, counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k,
            _ptr(pks) if n else None, _ptr(inf), _ptr(m), _ptr(off), stride, mlen, AGG_CHECK if check else 0,
            _ptr(wire) if k else None, _ptr(results) if k else None, _ptr(status) if n else None, C.byref(nfail)),
            "ssa_aggregates_many")
        return counts, wire[:-1], results, status, int(nfail.value)

    def aggregates(self, batches, check=False, counts=None, pk_inf=None, offsets=None):
        """aggregates_wire with the output split -> (list of AggregateSignature, None where the batch is refused;
        results uint32[k]; per-lane status uint8[N]; n_fail): for each batch what aggregate() gives it alone, from one
        call"""
        counts, wire, results, status, nfail = self.aggregates_wire(batches, check, counts, pk_inf, offsets)
        aggs = [AggregateSignature(a.tobytes()) if r == OK else None
                for a, r in zip(split_aggregates(counts, wire), results)]
        return aggs, results, status, nfail

    def aggregates_device(self, d_sigs, counts, d_pks, d_msgs, d_aggs=None, d_results=None, d_status=None, d_nfail=None,
                          d_pk_inf=None, d_offsets=None, msg_len=None, msg_stride=None, check=False):
        """device form over torch tensors on this engine's device, arguments as verify_aggregates_device takes them:
        counts a HOST sequence, d_sigs the (N, 81) signatures.  Without check it only enqueues.  The aggregates land in
        d_aggs (uint8[49 N + 32 k]), the results in d_results (int32[k]), the statuses in d_status (uint8[N]) and the
        count of failing lanes in d_nfail (int64[1]); each is allocated when None.  Returns the four tensors."""
        import torch
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        k, n = counts.size, int(counts.sum())
        dev = d_pks.device
        if d_aggs is None:
            d_aggs = torch.empty(49 * n + 32 * k + 4, dtype=torch.uint8, device=dev)[:49 * n + 32 * k]
        if d_results is None:
            d_results = torch.empty(max(k, 1), dtype=torch.int32, device=dev)[:k]
        if d_status is None:
            d_status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
        if d_nfail is None:
            d_nfail = torch.empty(1, dtype=torch.int64, device=dev)
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
        _check(_lib.ssa_aggregates_many_device(
            self._ctx, _addr(d_sigs), counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k, _addr(d_pks),
            _addr(d_pk_inf), _addr(d_msgs), _addr(d_offsets), stride, mlen, AGG_CHECK if check else 0,
            d_aggs.data_ptr() if k else None, _addr(d_results), _addr(d_status), d_nfail.data_ptr()),
            "ssa_aggregates_many_device")
        return d_aggs, d_results, d_status, d_nfail

    # ---- many aggregates through a key cache (include/schnorr_sig_amd.h) ----
    def verify_aggregates_cached(self, cache, aggregates, keys, msgs, pk_inf=None, offsets=None):
        """verify_aggregates with the key cache in front and the subgroup check of every key included -> (uint32[k],
        stats uint64[8]).  keys: (N, 96) affine keys with an affine cache, (N, 49) compressed keys with a cache made with
        wire=True (then pk_inf must be None: the wire form carries the flag).  An aggregate that holds a key outside the
        prime-order subgroup is answered INVALID_PUBLIC_KEY; every other verdict is the one verify_aggregate gives that
        aggregate alone, in every state of the cache.  stats: [0] distinct keys, [1] found in the cache, [2] checked and
        inserted, [3] automatic clears or compactions, [4] slices that bypassed the cache, [5] lanes at the probe bound
        plus rows that could not be published, [6] aggregates answered INVALID_PUBLIC_KEY."""
        counts, wire = pack_aggregates(aggregates)
        n, k = int(counts.sum()), counts.size
        width = 49 if cache.wire else 96
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        if keys.ndim != 2 and keys.size:
            raise ValueError("keys must be an (N, %d) array" % width)
        if keys.size and keys.shape[1] != width:
            raise ValueError("a %s key cache takes (N, %d) keys, not (N, %d)"
                             % ("wire" if cache.wire else "affine", width, keys.shape[1]))
        if cache.wire and pk_inf is not None:
            raise ValueError("pk_inf does not go with wire keys: the 49 bytes carry the identity flag")
        keys = keys.reshape(-1, width)
        if keys.shape[0] != n:
            raise MalformedInput("We should have the same number of signatures than public keys")
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        if inf is not None and inf.size != n:
            raise ValueError("pk_inf needs one byte per key")
        m, off, stride, mlen = self._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        out = np.full(k, 255, dtype=np.uint32)
        stats = np.zeros(8, dtype=np.uint64)
        head = (self._ctx, cache.handle, _ptr(wire) if k else None,
                counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k, _ptr(keys) if n else None)
        tail = (_ptr(m), _ptr(off), stride, mlen, _ptr(out) if k else None, stats.ctypes.data)
        if cache.wire:
            _check(_lib.ssa_verify_aggregates_many_cached_wire(*head, *tail), "ssa_verify_aggregates_many_cached_wire")
        else:
            _check(_lib.ssa_verify_aggregates_many_cached(*head, _ptr(inf), *tail), "ssa_verify_aggregates_many_cached")
        return out, stats

    def verify_aggregates_cached_device(self, cache, d_aggs, counts, d_keys, d_msgs, d_verdicts=None, d_pk_inf=None,
                                        d_offsets=None, msg_len=None, msg_stride=None, want_stats=True):
        """device form over torch tensors, as verify_aggregates_device: d_keys holds N x 96 or (wire cache) N x 49 bytes.
        One synchronisation per slice of SSA_LANE_SLICE lanes (the key dedup's); the aggregate stages are only enqueued,
        and with want_stats the call waits once more for the two words the device counts.  -> (d_verdicts, stats or
        None)"""
        import torch
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        k, n = counts.size, int(counts.sum())
        if cache.wire and d_pk_inf is not None:
            raise ValueError("pk_inf does not go with wire keys: the 49 bytes carry the identity flag")
        # the kernels read width * N key bytes and N flags: a tensor of the other mode's width would be read past its end
        width = 49 if cache.wire else 96
        have = 0 if d_keys is None else d_keys.numel() * d_keys.element_size()
        if have != n * width:
            raise ValueError("a %s key cache takes %d key bytes for %d lanes, not %d"
                             % ("wire" if cache.wire else "affine", n * width, n, have))
        if d_pk_inf is not None and d_pk_inf.numel() * d_pk_inf.element_size() != n:
            raise ValueError("pk_inf needs one byte per key")
        if d_verdicts is None:
            d_verdicts = torch.empty(max(k, 1), dtype=torch.int32, device=d_aggs.device)[:k]
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride, no_msgs_ok=True)
        stats = np.zeros(8, dtype=np.uint64) if want_stats else None
        head = (self._ctx, cache.handle, _addr(d_aggs), counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k,
                _addr(d_keys))
        tail = (_addr(d_msgs), _addr(d_offsets), stride, mlen, _addr(d_verdicts), stats.ctypes.data if want_stats else None)
        if cache.wire:
            _check(_lib.ssa_verify_aggregates_many_cached_wire_device(*head, *tail),
                   "ssa_verify_aggregates_many_cached_wire_device")
        else:
            _check(_lib.ssa_verify_aggregates_many_cached_device(*head, _addr(d_pk_inf), *tail),
                   "ssa_verify_aggregates_many_cached_device")
        return d_verdicts, stats

    def aggregates_coeffs(self, aggregates, pks, msgs, offsets=None):
        """tests: the coefficients of all N lanes as verify_aggregates derives them -> uint8[N, 16]"""
        counts, wire, pks, m, off, stride, mlen, _ = self._aggs_batch(aggregates, pks, msgs, offsets, None)
        out = np.zeros((pks.shape[0], 16), dtype=np.uint8)
        if pks.shape[0]:
            _check(_lib.ssa_debug_aggregates_many_coeffs(
                self._ctx, _ptr(wire), counts.ctypes.data_as(C.POINTER(C.c_uint64)), counts.size, _ptr(pks), _ptr(m),
                _ptr(off), stride, mlen, _ptr(out)), "ssa_debug_aggregates_many_coeffs")
        return out

    def debug_chacha20(self, key32, nonce12, counter0, n_blocks):
        """keystream blocks of the generator the MSM coefficients come from (RFC 8439 block function)"""
        key, nonce = _np_u8(bytearray(key32)), _np_u8(bytearray(nonce12))
        assert key.size == 32 and nonce.size == 12
        out = np.zeros(64 * n_blocks, dtype=np.uint8)
        _check(_lib.ssa_debug_chacha20(self._ctx, _ptr(key), _ptr(nonce), C.c_uint32(counter0), C.c_size_t(n_blocks),
                                       _ptr(out)), "ssa_debug_chacha20")
        return out.tobytes()

    def verify_one(self, sig81, pk96, message, check_torsion=True, pk_is_identity=False):
        sig, pk = _np_u8(bytearray(sig81)), _np_u8(bytearray(pk96))
        msg = _np_u8(bytearray(bytes(message) + b"\0"))
        if pk_is_identity:   # ssa_verify has no identity marker: one-element ssa_verify_many
            st, _ = self.verify_many(sig, pk, msg, offsets=np.array([0, len(message)], np.uint64),
                                     check_torsion=check_torsion, pk_inf=np.ones(1, np.uint8))
            return int(st[0])
        return _check(_lib.ssa_verify(self._ctx, _ptr(sig), _ptr(pk), _ptr(msg), len(message),
                                      FLAG_CHECK_TORSION if check_torsion else 0), "ssa_verify")

    def hash_message_many(self, sigs, pks, msgs, offsets=None):
        sigs, pks = _np_u8(sigs, 81), _np_u8(pks, 96)
        n = sigs.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(_lib.ssa_hash_message_many(self._ctx, _ptr(sigs), _ptr(pks), _ptr(m), _ptr(off), stride, mlen, n,
                                          _ptr(out)), "ssa_hash_message_many")
        return out

    def rescue_hash_many(self, felts):
        f = np.ascontiguousarray(felts, dtype=np.uint64)
        assert f.ndim == 2
        out = np.zeros((f.shape[0], 4), dtype=np.uint64)
        _check(_lib.ssa_rescue_hash_many(self._ctx, _ptr(f), f.shape[1], f.shape[0], _ptr(out)),
               "ssa_rescue_hash_many")
        return out

    def keygen_sign_many(self, sks, nonces, msgs, offsets=None, constant_time=False, keyed=False):
        """pk_i = [sk_i]G and sig_i = sign(sk_i, nonce_i, msg_i) -> (pks uint8[n, 96], sigs uint8[n, 81]).
        constant_time: SSA_FLAG_SIGN_CT (same bytes, no secret-dependent branch or address).
        keyed: the second array holds 130-byte KeyedSignature records pk(49) || sig(81) instead."""
        sks, nonces = _np_u8(sks, 32), _np_u8(nonces, 32)
        n = sks.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        pks = np.zeros((n, 96), dtype=np.uint8)
        sigs = np.zeros((n, 130 if keyed else 81), dtype=np.uint8)
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_keygen_sign_many_ex(self._ctx, _ptr(sks), _ptr(nonces), _ptr(m), _ptr(off), stride, mlen, n,
                                            flags, _ptr(pks), _ptr(sigs)), "ssa_keygen_sign_many_ex")
        return pks, sigs

    def pubkey_many(self, sks):
        """PublicKey::from(&PrivateKey) for n canonical non-zero scalars -> uint8[n, 96]: one constant-time base
        multiplication per key, nothing else derived from the secret (ssa_pubkey_many)"""
        sks = _np_u8(sks, 32)
        n = sks.shape[0]
        pks = np.zeros((n, 96), dtype=np.uint8)
        _check(_lib.ssa_pubkey_many(self._ctx, _ptr(sks), n, _ptr(pks)), "ssa_pubkey_many")
        return pks

    def pubkey_many_device(self, d_sks, n, d_pks):
        _check(_lib.ssa_pubkey_many_device(self._ctx, C.c_void_p(d_sks), n, C.c_void_p(d_pks)), "ssa_pubkey_many_device")

    def compress_many(self, pks, pk_inf=None):
        """PublicKey::to_bytes for n affine keys -> (uint8[n, 49], status uint8[n])"""
        pks = _np_u8(pks, 96)
        n = pks.shape[0]
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        out = np.zeros((n, 49), dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        _check(_lib.ssa_compress_many(self._ctx, _ptr(pks), _ptr(inf), n, _ptr(out), _ptr(st)), "ssa_compress_many")
        return out, st

    def verify_keyed_many(self, keyed, msgs, offsets=None, check_torsion=True):
        """n x KeyedSignature::verify on 130-byte records pk(49) || sig(81) -> (status, n_fail)."""
        kd = _np_u8(keyed, 130)
        n = kd.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        _check(_lib.ssa_verify_keyed_many(self._ctx, _ptr(kd), _ptr(m), _ptr(off), stride, mlen, n,
                                          FLAG_CHECK_TORSION if check_torsion else 0, _ptr(status),
                                          C.byref(nfail)), "ssa_verify_keyed_many")
        return status, int(nfail.value)

    def decompress_many(self, compressed):
        """n x 49-byte compressed points -> (pks uint8[n,96], is_identity uint8[n], status uint8[n])."""
        c = _np_u8(compressed, 49)
        n = c.shape[0]
        pks = np.zeros((n, 96), dtype=np.uint8)
        inf = np.zeros(n, dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        _check(_lib.ssa_decompress_many(self._ctx, _ptr(c), n, _ptr(pks), _ptr(inf), _ptr(st)),
               "ssa_decompress_many")
        return pks, inf, st

    # ---- hierarchical key derivation (src/derivation.rs) ------------------------------------
    @staticmethod
    def _derive_idx(indices, parent_idx, m):
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        pidx = None if parent_idx is None else np.ascontiguousarray(parent_idx, dtype=np.uint32).reshape(-1)
        if pidx is not None and pidx.shape[0] != idx.shape[0]:
            raise ValueError("parent_idx needs one entry per index")
        return idx, pidx

    def xprv_master_many(self, seeds):
        """ExtendedPrivateKey::generate_master_key for n 32-byte seeds -> (xprvs uint8[n, 64], status uint8[n])"""
        sd = _np_u8(seeds, 32)
        n = sd.shape[0]
        out = np.zeros((n, 64), dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        _check(_lib.ssa_xprv_master_many(self._ctx, _ptr(sd), n, _ptr(out), _ptr(st)), "ssa_xprv_master_many")
        return out, st

    def xprv_master_many_device(self, d_seeds, n, d_out, d_status):
        _check(_lib.ssa_xprv_master_many_device(self._ctx, d_seeds, n, d_out, d_status), "ssa_xprv_master_many_device")

    def xprv_derive_many(self, parents, indices, parent_idx=None, derive_public=False):
        """derive_private (or derive_public) of m 64-byte xprvs -> (children uint8[n, 64] (or [n, 81]), status uint8[n]).
        parent_idx None: one parent for every child (m == 1) or one per child (m == n)."""
        par = _np_u8(parents, 64)
        idx, pidx = self._derive_idx(indices, parent_idx, par.shape[0])
        n = idx.shape[0]
        out = np.zeros((n, 81 if derive_public else 64), dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        _check(_lib.ssa_xprv_derive_many(self._ctx, _ptr(par), par.shape[0], _ptr(pidx), _ptr(idx), n,
                                         FLAG_DERIVE_PUBLIC if derive_public else 0, _ptr(out), _ptr(st)),
               "ssa_xprv_derive_many")
        return out, st

    def xprv_derive_many_device(self, d_parents, m, d_indices, n, d_children, d_status, d_parent_idx=0,
                                derive_public=False):
        _check(_lib.ssa_xprv_derive_many_device(self._ctx, d_parents, m, d_parent_idx or None, d_indices, n,
                                                FLAG_DERIVE_PUBLIC if derive_public else 0, d_children, d_status),
               "ssa_xprv_derive_many_device")

    def xpub_derive_many(self, parents, indices, parent_idx=None):
        """derive_normal_public of m 81-byte xpubs -> (children uint8[n, 81], pks uint8[n, 96] (affine, zero for the
        identity), is_identity uint8[n], status uint8[n])"""
        par = _np_u8(parents, 81)
        idx, pidx = self._derive_idx(indices, parent_idx, par.shape[0])
        n = idx.shape[0]
        out = np.zeros((n, 81), dtype=np.uint8)
        pks = np.zeros((n, 96), dtype=np.uint8)
        inf = np.zeros(n, dtype=np.uint8)
        st = np.full(n, 255, dtype=np.uint8)
        _check(_lib.ssa_xpub_derive_many(self._ctx, _ptr(par), par.shape[0], _ptr(pidx), _ptr(idx), n, _ptr(out),
                                         _ptr(pks), _ptr(inf), _ptr(st)), "ssa_xpub_derive_many")
        return out, pks, inf, st

    def xpub_derive_many_device(self, d_parents, m, d_indices, n, d_children, d_status, d_parent_idx=0, d_pks=0,
                                d_pk_inf=0):
        _check(_lib.ssa_xpub_derive_many_device(self._ctx, d_parents, m, d_parent_idx or None, d_indices, n, d_children,
                                                d_pks or None, d_pk_inf or None, d_status),
               "ssa_xpub_derive_many_device")

    def debug_hmac_sha512(self, key, msgs):
        """HMAC-SHA512(key, msgs[i]) on the GPU for n messages of one length (<= 239 bytes; key <= 256 bytes)
        -> uint8[n, 64]"""
        k = np.frombuffer(bytes(key) + b"\0", np.uint8).copy()
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        if m.ndim == 1:
            m = m.reshape(1, -1)
        n, ml = m.shape
        flat = np.concatenate([m.reshape(-1), np.zeros(1, np.uint8)])
        out = np.zeros((n, 64), dtype=np.uint8)
        _check(_lib.ssa_debug_hmac_sha512(self._ctx, _ptr(k), len(bytes(key)), _ptr(flat), ml, n, _ptr(out)),
               "ssa_debug_hmac_sha512")
        return out

    # ---- keyed context (many signatures by few signers) ---------------------------------
    def keyset_create(self, pks, pk_inf=None, kind="auto"):
        """-> KeySet: subgroup check and tables done once per key.  kind: "auto" (combs while they fit the context's HBM
        budget, else -- or when their allocation fails -- the ladder tables), "comb" (100 MB per key, no doublings at
        verification time) or "ladder" (4 KB per key)"""
        pks = _np_u8(pks, 96)
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        ks = C.c_void_p()
        _check(_lib.ssa_keyset_create(self._ctx, _ptr(pks), _ptr(inf), pks.shape[0], KEYSET_KINDS[kind], C.byref(ks)),
               "ssa_keyset_create")
        return KeySet(self, ks, pks.shape[0])

    def keyset_create_device(self, d_pks, m, d_pk_inf=0, kind="auto"):
        ks = C.c_void_p()
        _check(_lib.ssa_keyset_create_device(self._ctx, d_pks, d_pk_inf or None, m, KEYSET_KINDS[kind], C.byref(ks)),
               "ssa_keyset_create_device")
        return KeySet(self, ks, m)

    def keyset_destroy(self, ks):
        ks.close()

    def keyset_status(self, ks, m=None):
        st = np.full(ks.m if m is None else m, 255, dtype=np.uint8)
        _check(_lib.ssa_keyset_status(ks.handle, _ptr(st)), "ssa_keyset_status")
        return st

    def verify_many_indexed(self, ks, key_idx, sigs, msgs, offsets=None, check_torsion=True, sig_flag_byte=False):
        """n x Signature::verify against key key_idx[i] of the key set -> (status uint8[n], n_fail)"""
        sigs = _np_u8(sigs, 81)
        n = sigs.shape[0]
        idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
        assert idx.size == n
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        flags = (FLAG_CHECK_TORSION if check_torsion else 0) | (FLAG_SIG_FLAG_BYTE if sig_flag_byte else 0)
        _check(_lib.ssa_verify_many_indexed(self._ctx, ks.handle, _ptr(idx), _ptr(sigs), _ptr(m), _ptr(off), stride, mlen, n,
                                            flags, _ptr(status), C.byref(nfail)), "ssa_verify_many_indexed")
        return status, int(nfail.value)

    def verify_many_indexed_device(self, ks, d_key_idx, d_sigs, d_msgs, n, msg_len, d_status, d_nfail, msg_stride=None,
                                   d_offsets=0, check_torsion=True):
        _check(_lib.ssa_verify_many_indexed_device(self._ctx, ks.handle, d_key_idx, d_sigs, d_msgs, d_offsets or None,
                                                   msg_stride if msg_stride is not None else msg_len, msg_len, n,
                                                   FLAG_CHECK_TORSION if check_torsion else 0, d_status, d_nfail),
               "ssa_verify_many_indexed_device")

    # ---- signer sets (KeyPair::sign for many messages by few key pairs) ---------------------
    def signer_set_create(self, sks):
        """-> SignerSet holding the key pairs of m canonical non-zero secret keys (uint8[m, 32]) on the device"""
        sks = _np_u8(sks, 32)
        ss = C.c_void_p()
        _check(_lib.ssa_signer_set_create(self._ctx, _ptr(sks), sks.shape[0], C.byref(ss)), "ssa_signer_set_create")
        return SignerSet(self, ss, sks.shape[0])

    def signer_set_create_device(self, d_sks, m, sk_stride=32):
        """key k at d_sks + k * sk_stride (64: the key half of ExtendedPrivateKey records); a zero or non-canonical
        key gets status 3 (signer_set_status)"""
        ss = C.c_void_p()
        _check(_lib.ssa_signer_set_create_device(self._ctx, C.c_void_p(d_sks), sk_stride, m, C.byref(ss)),
               "ssa_signer_set_create_device")
        return SignerSet(self, ss, m)

    def signer_set_status(self, ss):
        st = np.full(ss.m, 255, dtype=np.uint8)
        _check(_lib.ssa_signer_set_status(ss.handle, _ptr(st)), "ssa_signer_set_status")
        return st

    def signer_set_public_keys(self, ss):
        """-> (uint8[m, 96] affine keys, uint8[m, 49] compressed keys)"""
        pks = np.zeros((ss.m, 96), dtype=np.uint8)
        cpks = np.zeros((ss.m, 49), dtype=np.uint8)
        _check(_lib.ssa_signer_set_public_keys(ss.handle, _ptr(pks), _ptr(cpks)), "ssa_signer_set_public_keys")
        return pks, cpks

    def sign_many_indexed(self, ss, key_idx, nonces, msgs, offsets=None, constant_time=False, keyed=False):
        """signature i by key pair key_idx[i] of the signer set with nonce i -> uint8[n, 81] (uint8[n, 130] keyed);
        byte for byte keygen_sign_many(sks[key_idx], nonces, msgs, ...)[1]"""
        idx = np.ascontiguousarray(key_idx, dtype=np.uint32).reshape(-1)
        nonces = _np_u8(nonces, 32)
        n = idx.shape[0]
        assert nonces.shape[0] == n
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        sigs = np.zeros((n, 130 if keyed else 81), dtype=np.uint8)
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_sign_many_indexed(self._ctx, ss.handle, _ptr(idx), _ptr(nonces), _ptr(m), _ptr(off), stride,
                                          mlen, n, flags, _ptr(sigs)), "ssa_sign_many_indexed")
        return sigs

    def sign_many_indexed_device(self, ss, d_key_idx, d_nonces, d_msgs, n, msg_len, d_sigs, d_status=0,
                                 msg_stride=None, d_offsets=0, constant_time=False, keyed=False):
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_sign_many_indexed_device(self._ctx, ss.handle, d_key_idx, d_nonces, d_msgs, d_offsets or None,
                                                 msg_stride if msg_stride is not None else msg_len, msg_len, n, flags,
                                                 d_sigs, d_status or None), "ssa_sign_many_indexed_device")

    # ---- nonces and keys drawn on the device (Scalar::random(rng) on the GPU: no nonce exists on the host) ------
    def keygen_sign_many_rng(self, sks, msgs, offsets=None, constant_time=False, keyed=False):
        """keygen_sign_many with the nonces drawn on the device -> (pks uint8[n, 96], sigs uint8[n, 81] or [n, 130])"""
        sks = _np_u8(sks, 32)
        n = sks.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        pks = np.zeros((n, 96), dtype=np.uint8)
        sigs = np.zeros((n, 130 if keyed else 81), dtype=np.uint8)
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_keygen_sign_many_rng(self._ctx, _ptr(sks), _ptr(m), _ptr(off), stride, mlen, n, flags, _ptr(pks),
                                             _ptr(sigs)), "ssa_keygen_sign_many_rng")
        return pks, sigs

    def keygen_sign_many_rng_device(self, d_sks, d_msgs, n, msg_len, d_pks, d_sigs, msg_stride=None, d_offsets=0,
                                    constant_time=False, keyed=False):
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_keygen_sign_many_rng_device(self._ctx, d_sks, d_msgs, d_offsets or None,
                                                    msg_stride if msg_stride is not None else msg_len, msg_len, n, flags,
                                                    d_pks or None, d_sigs), "ssa_keygen_sign_many_rng_device")

    def sign_many_indexed_rng(self, ss, key_idx, msgs, offsets=None, constant_time=False, keyed=False):
        """sign_many_indexed with the nonces drawn on the device -> uint8[n, 81] (uint8[n, 130] keyed)"""
        idx = np.ascontiguousarray(key_idx, dtype=np.uint32).reshape(-1)
        n = idx.shape[0]
        m, off, stride, mlen = self._msg_args(msgs, offsets, n)
        sigs = np.zeros((n, 130 if keyed else 81), dtype=np.uint8)
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_sign_many_indexed_rng(self._ctx, ss.handle, _ptr(idx), _ptr(m), _ptr(off), stride, mlen, n, flags,
                                              _ptr(sigs)), "ssa_sign_many_indexed_rng")
        return sigs

    def sign_many_indexed_rng_device(self, ss, d_key_idx, d_msgs, n, msg_len, d_sigs, d_status=0, msg_stride=None,
                                     d_offsets=0, constant_time=False, keyed=False):
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_sign_many_indexed_rng_device(self._ctx, ss.handle, d_key_idx, d_msgs, d_offsets or None,
                                                     msg_stride if msg_stride is not None else msg_len, msg_len, n,
                                                     flags, d_sigs, d_status or None), "ssa_sign_many_indexed_rng_device")

    def signer_set_generate(self, m):
        """KeyPair::new(rng) for m key pairs whose secret keys are drawn on the device -> SignerSet"""
        ss = C.c_void_p()
        _check(_lib.ssa_signer_set_generate(self._ctx, int(m), C.byref(ss)), "ssa_signer_set_generate")
        return SignerSet(self, ss, m)

    def signer_set_secret_keys(self, ss):
        """KeyPair::to_bytes for the whole set -> uint8[m, 32] (zeros for a malformed key)"""
        sks = np.zeros((ss.m, 32), dtype=np.uint8)
        _check(_lib.ssa_signer_set_secret_keys(ss.handle, _ptr(sks)), "ssa_signer_set_secret_keys")
        return sks

    def debug_pin_rng(self, seed44):
        """TESTS ONLY: every later draw on this engine uses seed44 (None unpins).  A pinned engine reuses its nonces,
        which gives the signing keys away."""
        if seed44 is None:
            _check(_lib.ssa_debug_pin_rng(self._ctx, None), "ssa_debug_pin_rng")
            return
        seed = _np_u8(bytearray(seed44))
        if seed.size != 44:
            raise ValueError("the seed is 44 bytes")
        _check(_lib.ssa_debug_pin_rng(self._ctx, _ptr(seed)), "ssa_debug_pin_rng")

    def debug_draw_scalars(self, blocks):
        """the device's draw rule on n block pairs B0 || B1 (uint8[n, 128]) -> uint8[n, 32]"""
        b = _np_u8(blocks, 128)
        out = np.zeros((b.shape[0], 32), dtype=np.uint8)
        _check(_lib.ssa_debug_draw_scalars(self._ctx, _ptr(b), b.shape[0], _ptr(out)), "ssa_debug_draw_scalars")
        return out

    # ---- device-buffer entry points (raw device addresses, e.g. torch.Tensor.data_ptr()) ----
    def set_stream(self, hip_stream):
        _check(_lib.ssa_ctx_set_stream(self._ctx, C.c_void_p(hip_stream or 0)), "ssa_ctx_set_stream")

    def sync(self):
        _check(_lib.ssa_ctx_sync(self._ctx), "ssa_ctx_sync")

    def stream_release(self, consumer_stream):
        """stream `consumer_stream` (a hipStream_t handle, e.g. torch.cuda.current_stream().cuda_stream) waits for
        everything this engine has enqueued so far: its outputs become visible there without a host synchronisation"""
        _check(_lib.ssa_ctx_stream_release(self._ctx, C.c_void_p(consumer_stream or 0)), "ssa_ctx_stream_release")

    def stream_acquire(self, producer_stream):
        """this engine's stream waits for everything enqueued on `producer_stream` so far (inputs written there, e.g.
        by a collective, are visible to the next call on the engine)"""
        _check(_lib.ssa_ctx_stream_acquire(self._ctx, C.c_void_p(producer_stream or 0)), "ssa_ctx_stream_acquire")

    def selfcheck(self):
        """ssa_ctx_selfcheck: the exact check of the comb for G and (once built) the constant-time table.  Returns the
        eight out[] fields by name (SELFCHECK_FIELDS) plus ok; a failing table is a result (ok False), not an exception.
        A comb that fails is retired: engines created afterwards build a new one, this one should be closed."""
        out = (C.c_uint64 * 8)()
        rc = _lib.ssa_ctx_selfcheck(self._ctx, 0, out)
        if rc != ERR_TABLE:
            _check(rc, "ssa_ctx_selfcheck")
        res = dict(zip(SELFCHECK_FIELDS, (int(v) for v in out)))
        res["ok"] = rc == OK
        return res

    def debug_table_read(self, which, first_row, n):
        """tests: rows [first_row, first_row + n) of a table (TABLE_COMB / TABLE_CT) as an (n, 12) uint64 array"""
        out = np.zeros((n, 12), dtype=np.uint64)
        _check(_lib.ssa_debug_table_read(self._ctx, int(which), int(first_row), int(n), _ptr(out)), "ssa_debug_table_read")
        return out

    def debug_table_xor(self, which, row, word, mask):
        """tests: XOR `mask` into one word of a table ON THE DEVICE.  The comb is shared by every engine of the process on
        this device and geometry; run no verification, signing or derivation on any of them afterwards."""
        _check(_lib.ssa_debug_table_xor(self._ctx, int(which), int(row), int(word), C.c_uint64(int(mask))),
               "ssa_debug_table_xor")

    def debug_fault_after_chunk(self, chunk):
        """tests: the NEXT pipelined host-buffer upload fails after chunk `chunk` (one shot; < 0 disarms)"""
        _check(_lib.ssa_debug_fault_after_chunk(self._ctx, int(chunk)), "ssa_debug_fault_after_chunk")

    def debug_poison_workspaces(self, byte):
        """tests: every workspace, staging and page-locked buffer of the context (and of its second set) filled with
        `byte` up to its capacity; the constant-time table and everything shared or handed out stay as they are"""
        _check(_lib.ssa_debug_poison_workspaces(self._ctx, int(byte)), "ssa_debug_poison_workspaces")

    def verify_many_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_status, d_nfail, msg_stride=None,
                           d_offsets=0, d_pk_inf=0, check_torsion=False, mode=None, sig_flag_byte=False):
        """sig_flag_byte=True with check_torsion=False is what ssa_verify_batch runs (src/batch.rs:104: R is decompressed
        with the flag byte of sig.x, no subgroup check)"""
        _check(_lib.ssa_verify_many_device(
            self._ctx, d_sigs, d_pks, *self._dev_batch(d_pk_inf, d_msgs, d_offsets, msg_stride, msg_len, n),
            self._verify_flags(check_torsion, sig_flag_byte, mode), d_status, d_nfail), "ssa_verify_many_device")

    def keygen_sign_many_device(self, d_sks, d_nonces, d_msgs, n, msg_len, d_pks, d_sigs, msg_stride=None,
                                d_offsets=0, constant_time=False, keyed=False):
        flags = (FLAG_SIGN_CT if constant_time else 0) | (FLAG_SIGN_KEYED if keyed else 0)
        _check(_lib.ssa_keygen_sign_many_ex_device(self._ctx, d_sks, d_nonces, d_msgs, d_offsets or None,
                                                   msg_stride if msg_stride is not None else msg_len, msg_len, n, flags,
                                                   d_pks or None, d_sigs), "ssa_keygen_sign_many_ex_device")

    def compress_many_device(self, d_pks, n, d_out, d_pk_inf=0, d_status=0):
        _check(_lib.ssa_compress_many_device(self._ctx, d_pks, d_pk_inf or None, n, d_out, d_status or None),
               "ssa_compress_many_device")

    def rescue_hash_many_device(self, d_felts, per_row, n, d_out):
        _check(_lib.ssa_rescue_hash_many_device(self._ctx, d_felts, per_row, n, d_out),
               "ssa_rescue_hash_many_device")

    def hash_message_many_device(self, d_sigs, d_pks, d_msgs, n, msg_len, d_out, msg_stride=None, d_offsets=0):
        _check(_lib.ssa_hash_message_many_device(self._ctx, d_sigs, d_pks, d_msgs, d_offsets or None,
                                                 msg_stride if msg_stride is not None else msg_len, msg_len, n,
                                                 d_out), "ssa_hash_message_many_device")

    def enable_timing(self, on=True):
        _check(_lib.ssa_ctx_enable_timing(self._ctx, int(on)), "ssa_ctx_enable_timing")

    def read_timing(self, kernel):
        avg = C.c_double(0)
        cnt = C.c_uint64(0)
        _check(_lib.ssa_ctx_read_timing(self._ctx, kernel.encode(), C.byref(avg), C.byref(cnt)),
               "ssa_ctx_read_timing")
        return avg.value, int(cnt.value)

    def debug_split_config(self, split_min=-1, split_frac=-1, tail_b=-1, alone=-1):
        """tests: the knobs of the one-slice split on this context (SSA_SPLIT_MIN, SSA_SPLIT_FRAC in 1/16ths with 0 = off,
        SSA_SPLIT_TAIL_B, SSA_SPLIT_ALONE); a negative value leaves that knob as it is"""
        _check(_lib.ssa_debug_split_config(self._ctx, int(split_min), int(split_frac), int(tail_b), int(alone)),
               "ssa_debug_split_config")

    def debug_split_timing(self, kernel):
        """tests: (span, part A, part B) in ms of the last entry a split call recorded under `kernel`, left in place for
        read_timing; None when there is none"""
        out = np.zeros(3, dtype=np.float64)
        rc = _lib.ssa_debug_split_timing(self._ctx, kernel.encode(), out.ctypes.data)
        if rc == ERR_ARG:
            return None
        _check(rc, "ssa_debug_split_timing")
        return tuple(float(v) for v in out)

    def host_path_probe(self, sigs_t, pks_t, msgs_t, n, reps=3):
        """PCIe-inclusive rate of the host-buffer entry point ssa_verify_many (what a Rust shim binds): the
        device tensors are copied to ordinary pageable host arrays first, then `reps` timed calls."""
        import time
        hs, hp, hm = (t[:n].cpu().numpy() for t in (sigs_t, pks_t, msgs_t))
        st, nf = self.verify_many(hs, hp, hm, check_torsion=False, mode="lane", sig_flag_byte=True)     # warm-up: workspaces
        t0 = time.perf_counter()
        for _ in range(reps):
            st, nf = self.verify_many(hs, hp, hm, check_torsion=False, mode="lane", sig_flag_byte=True)
        dt = (time.perf_counter() - t0) / reps
        verdict = self.verify_batch_msm(hs, hp, hm)                                  # MSM form, library-drawn coefficients
        t0 = time.perf_counter()
        for _ in range(reps):
            verdict = self.verify_batch_msm(hs, hp, hm)
        dt_msm = (time.perf_counter() - t0) / reps
        return {"entry_point": "ssa_verify_many (host buffers in pageable memory, copied through the library's page-locked "
                               "bounce buffers, uploads in chunks overlapped with the hash kernel)",
                "ms_per_batch": dt * 1e3, "verifications_per_sec": n / dt, "rejected": int(nf),
                "verify_batch_msm_ms_per_batch": dt_msm * 1e3, "verify_batch_msm_signatures_per_sec": n / dt_msm,
                "verify_batch_msm_verdict": int(verdict)}

    # ---- probes --------------------------------------------------------------------------
    def debug_arith(self, op, a, b, out_cols):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
        n = a.shape[0]
        out = np.zeros((n, out_cols), dtype=np.uint64)
        _check(_lib.ssa_debug_arith(self._ctx, op, _ptr(a), _ptr(b), n, a.shape[1],
                                    b.shape[1] if b is not None else 0, _ptr(out), out_cols), "ssa_debug_arith")
        return out

    def bench_fpmul(self, variant):
        v = C.c_double(0)
        _check(_lib.ssa_bench_fpmul(self._ctx, variant, C.byref(v)), "ssa_bench_fpmul")
        return v.value


def debug_corrupt_table_builds(n):
    """tests: the next n comb builds of this process get one word flipped before their check (0 disarms)"""
    _check(_lib.ssa_debug_corrupt_table_builds(int(n)), "ssa_debug_corrupt_table_builds")


KEYCHECK_DEEP, KEYCHECK_REPAIR = 1, 2      # SSA_KEYCHECK_*
KEYCHECK_FIELDS = ("keys_checked", "keys_bad", "first_bad_key", "ladder_entries_checked", "comb_rows_checked",
                   "keys_rebuilt_and_compared", "combs_skipped", "rows_repaired")
# `what` of ssa_debug_keytab_xor / _read: the target and the words a read returns
KEYTAB_LADDER, KEYTAB_STATUS, KEYTAB_KEY, KEYTAB_PK_INF, KEYTAB_COMB = 0, 1, 2, 3, 4
KEYTAB_WIRE = 5     # key caches in wire mode: the row's 49 compressed bytes as seven words (six of x, one holding the flag byte)
_KEYTAB_READ_WORDS = {KEYTAB_LADDER: 512, KEYTAB_STATUS: 1, KEYTAB_KEY: 12, KEYTAB_PK_INF: 1, KEYTAB_COMB: 24,
                      KEYTAB_WIRE: 7}
KEYCACHE_WIRE = 1   # SSA_KEYCACHE_WIRE
KEYCACHE_EVICT = {"clear": 0, "recent": 1}   # SSA_KEYCACHE_EVICT_CLEAR / _RECENT


def _keycheck_result(rc, out, what):
    """the eight out[] fields by name plus ok; failing keys are a result (ok False), not an exception"""
    if rc != ERR_TABLE:
        _check(rc, what)
    res = dict(zip(KEYCHECK_FIELDS, (int(v) for v in out)))
    res["ok"] = rc == OK
    return res


class _KeyTables:
    """what KeySet and KeyCache share: the self-check of their per-key tables and its test hooks"""

    def _pair(self):
        """(key set handle, key cache handle): exactly one is set"""
        raise NotImplementedError

    def debug_keytab_xor(self, what, key, word, mask):
        """tests: XOR `mask` into one word (or the one byte) of a key's row ON THE DEVICE.  Only selfcheck, its repair and
        close may run on the object afterwards."""
        ks, kc = self._pair()
        _check(_lib.ssa_debug_keytab_xor(ks, kc, int(what), int(key), int(word), C.c_uint64(int(mask))),
               "ssa_debug_keytab_xor")

    def debug_keytab_read(self, what, key):
        """tests: a key's ladder table (512 words), status byte, key words (12), pk_inf byte or first two comb rows"""
        ks, kc = self._pair()
        out = np.zeros(_KEYTAB_READ_WORDS[int(what)], dtype=np.uint64)
        _check(_lib.ssa_debug_keytab_read(ks, kc, int(what), int(key), _ptr(out)), "ssa_debug_keytab_read")
        return out


class KeySet(_KeyTables):
    """ssa_keyset handle tied to its Engine: the engine cannot be collected before the key set, and the handle is
    destroyed exactly once (close(), or when the object goes away)."""

    def __init__(self, engine, handle, m):
        self.engine = engine      # keeps the context alive
        self.handle = handle
        self.m = int(m)

    def _pair(self):
        return self.handle, None

    def selfcheck(self, deep=False):
        """ssa_keyset_selfcheck: the exact check of every key's ladder table, status and (comb mode) comb against the
        stored key bytes.  deep=True also recomputes [q]P per key: without it a status flipped between 0 and 1 is not
        seen.  -> the KEYCHECK_FIELDS by name, ok, and bad: a uint8[m] with 1 per failing key (hand those in again)."""
        out = (C.c_uint64 * 8)()
        bad = np.zeros(self.m, dtype=np.uint8)
        rc = _lib.ssa_keyset_selfcheck(self.handle, KEYCHECK_DEEP if deep else 0, _ptr(bad), out)
        res = _keycheck_result(rc, out, "ssa_keyset_selfcheck")
        res["bad"] = bad
        return res

    def close(self):
        if self.handle:
            _lib.ssa_keyset_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """a device object (ssa_<_prefix>_* of the ABI) tied to its Engine like KeySet: destroyed exactly once, by close(),
    the end of a `with` block, or when the object goes away"""
    _prefix = None

    def __init__(self, engine, handle):
        self.engine = engine      # keeps the context alive
        self.handle = handle

    def _call(self, what, *args):
        name = "ssa_%s_%s" % (self._prefix, what)
        return _check(getattr(_lib, name)(*args), name)

    def close(self):
        if self.handle:
            getattr(_lib, "ssa_%s_destroy" % self._prefix)(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyCache(_Handle, _KeyTables):
    """ssa_keycache handle (Engine.keycache_create): checked public keys, their statuses and tables, kept on the device
    across slices and calls of verify_many_cached.  Tied to its Engine like KeySet; destroyed exactly once (close(), the
    end of a `with` block, or when the object goes away)."""
    _prefix = "keycache"

    def __init__(self, engine, handle, wire=False):
        super().__init__(engine, handle)
        self.wire = bool(wire)    # rows identified by the 49 compressed key bytes

    def info(self):
        """{'capacity', 'held', 'clears', 'device_bytes'}"""
        out = (C.c_uint64 * 4)()
        _check(_lib.ssa_keycache_info(self.handle, out), "ssa_keycache_info")
        return {"capacity": int(out[0]), "held": int(out[1]), "clears": int(out[2]), "device_bytes": int(out[3])}

    def set_eviction(self, policy):
        """ssa_keycache_set_eviction: "clear" (the default: a full cache clears itself) or "recent" (a full cache keeps
        the rows used most recently: DESIGN.md section 19).  "recent" allocates the rows' stamps and the compaction's
        scratch, once: info()["device_bytes"] grows here and never again."""
        if policy not in KEYCACHE_EVICT:
            raise ValueError("policy must be one of %s" % sorted(KEYCACHE_EVICT))
        _check(_lib.ssa_keycache_set_eviction(self.handle, KEYCACHE_EVICT[policy]), "ssa_keycache_set_eviction")

    def eviction_info(self):
        """{'policy' ("clear" / "recent"), 'compactions', 'dropped', 'last_kept', 'last_moved', 'epoch'}"""
        out = (C.c_uint64 * 8)()
        _check(_lib.ssa_keycache_eviction_info(self.handle, out), "ssa_keycache_eviction_info")
        names = {v: k for k, v in KEYCACHE_EVICT.items()}
        return {"policy": names[int(out[0])], "compactions": int(out[1]), "dropped": int(out[2]),
                "last_kept": int(out[3]), "last_moved": int(out[4]), "epoch": int(out[5])}

    def _pair(self):
        return None, self.handle

    def selfcheck(self, deep=False, repair=False):
        """ssa_keycache_selfcheck: the exact check of every held row (ladder table and status against the row's stored
        key bytes).  deep=True also recomputes [q]P per key; repair=True rebuilds failing rows in place from their
        stored bytes and checks again (ok is then True when the cache is clean afterwards).  -> the KEYCHECK_FIELDS by
        name plus ok."""
        out = (C.c_uint64 * 8)()
        flags = (KEYCHECK_DEEP if deep else 0) | (KEYCHECK_REPAIR if repair else 0)
        return _keycheck_result(_lib.ssa_keycache_selfcheck(self.handle, flags, out), out, "ssa_keycache_selfcheck")

    def clear(self):
        """forget every key: the next call is cold"""
        _check(_lib.ssa_keycache_clear(self.handle), "ssa_keycache_clear")


AGGR_NO_SCREEN = 1    # SSA_AGGR_NO_SCREEN
AGGR_HOLD_KEYS49 = 2  # SSA_AGGR_HOLD_KEYS49
AGGR_HOLD_ADMISSION = 8  # SSA_AGGR_HOLD_ADMISSION
AGGR_HOLD_INDEX = 32  # SSA_AGGR_HOLD_INDEX
# the eight words of Aggregator.index_info
AGGREGATOR_INDEX_FIELDS = ("slots", "indexed", "stale", "rebuilds", "overflowed", "lookups", "ids", "reserved")
# the admission classes an Aggregator made with hold_admission=True records
ADM_UNSCREENED = 0    # SSA_ADM_UNSCREENED: push(screen=False)
ADM_SCREENED = 1      # SSA_ADM_SCREENED: the plain screened push
ADM_KEY_CHECKED = 2   # SSA_ADM_KEY_CHECKED: push(cache=), push_keyed
AGGREGATOR_FIELDS = ("held", "capacity", "block_lanes", "pushes", "offered", "dropped", "blocks", "finishes")
AGGVERIFIER_FIELDS = ("held", "capacity", "block_lanes", "pushes", "pushed", "reserved", "blocks", "finishes")
#   ("reserved" is word [5] of ssa_aggverifier_info: since section 29 the lanes pushed through a key cache, 0 for an
#    object that sees plain pushes only; the name stays, AggregateVerifier.cached_lanes() reads it)
AGGREGATOR_ALL = (1 << (8 * C.sizeof(C.c_size_t))) - 1      # SIZE_MAX: finish every lane held


def aggverifier_key_span():
    """tests: AGV_KST_SPAN, the lanes of key statuses one workgroup of the keyed finish's fold takes"""
    return int(_lib.ssa_debug_aggverifier_key_span())


def aggregator_plan(held, m, block_lanes=0):
    """tests: (first completed block, completed blocks, first lane of the ragged tail, its length) of a push of m kept
    lanes onto `held` lanes (ssa_debug_aggregator_plan: host code, no device)"""
    out = (C.c_uint64 * 4)()
    _check(_lib.ssa_debug_aggregator_plan(int(held), int(m), int(block_lanes), out), "ssa_debug_aggregator_plan")
    return tuple(int(v) for v in out)


def aggregator_bytes(capacity, block_lanes=0, hold_keys=False):
    """tests: the bytes Engine.aggregator allocates -- (R's, scalars, leaves, tops, key column), the last 0 without
    hold_keys (ssa_debug_aggregator_bytes: host code, no device)"""
    out = (C.c_uint64 * 5)()
    _check(_lib.ssa_debug_aggregator_bytes(int(capacity), int(block_lanes), AGGR_HOLD_KEYS49 if hold_keys else 0, out),
           "ssa_debug_aggregator_bytes")
    return tuple(int(v) for v in out)


def _aggr_flags(hold_keys, hold_admission, index=False):
    return ((AGGR_HOLD_KEYS49 if hold_keys else 0) | (AGGR_HOLD_ADMISSION if hold_admission else 0)
            | (AGGR_HOLD_INDEX if index else 0))


def aggregator_bytes_ex(capacity, block_lanes=0, hold_keys=False, hold_admission=False, index=False):
    """tests: the five words of aggregator_bytes, the admission column (0 without hold_admission), the leaf index (0
    without index) and a zero (ssa_debug_aggregator_bytes_ex: host code, no device)"""
    out = (C.c_uint64 * 8)()
    _check(_lib.ssa_debug_aggregator_bytes_ex(int(capacity), int(block_lanes),
                                              _aggr_flags(hold_keys, hold_admission, index), out),
           "ssa_debug_aggregator_bytes_ex")
    return tuple(int(v) for v in out)


def _require_class(require):
    """the `require` argument of a mixed push through a key cache: 0, 1 or 2 (ADM_*); ValueError before any call"""
    if isinstance(require, (bool, np.bool_)) or not isinstance(require, (int, np.integer)) or not 0 <= int(require) <= 2:
        raise ValueError("require is an admission class: 0, 1 or 2")
    return int(require)


def aggregator_remove_plan(held, first_changed, new_held, block_lanes=0):
    """tests: (blocks whose tops stay, blocks whose tops are moved, first block reduced again, blocks reduced again) of a
    removal that keeps new_held of `held` lanes and changes no place in front of first_changed; first_changed == 0
    stands for drop_front(held - new_held) (ssa_debug_aggregator_remove_plan: host code, no device)"""
    out = (C.c_uint64 * 4)()
    _check(_lib.ssa_debug_aggregator_remove_plan(int(held), int(first_changed), int(new_held), int(block_lanes), out),
           "ssa_debug_aggregator_remove_plan")
    return tuple(int(v) for v in out)


def _n_take(n_take):
    """the n_take argument of the ABI: None takes every lane held"""
    return AGGREGATOR_ALL if n_take is None else int(n_take)


def _order_u32(order):
    """a list of held lanes' places (any integer sequence or array) as the contiguous uint32 array the ABI takes;
    ValueError, before any call, for values that are no integers or do not fit 32 bits"""
    if isinstance(order, np.ndarray) and order.dtype == np.uint32 and order.ndim == 1 and order.flags.c_contiguous:
        return order
    a = np.asarray(order if isinstance(order, np.ndarray) else list(order))
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("order is a one-dimensional sequence of integers")
    if int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF:
        raise ValueError("order holds places of held lanes: 0 .. 2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32)


AGGV_UNKNOWN = 0xFFFFFFFF      # SSA_AGGV_UNKNOWN: the lane comes with the call, not from the pool


def _places_u32(places):
    """the places of a mixed push (any integer sequence or array; None or -1: an unknown lane) as the contiguous uint32
    array the ABI takes, AGGV_UNKNOWN for the unknown ones; ValueError, before any call, for values that are no
    integers or do not fit"""
    if isinstance(places, np.ndarray) and places.dtype == np.uint32 and places.ndim == 1 and places.flags.c_contiguous:
        return places
    if isinstance(places, np.ndarray):
        if places.ndim != 1 or places.dtype.kind not in "iu":
            raise ValueError("places is a one-dimensional sequence of integers")
        vals = places.astype(object).tolist() if places.size else []
    else:
        vals = list(places)
    out = np.empty(len(vals), dtype=np.uint32)
    for i, v in enumerate(vals):
        if v is None:
            v = AGGV_UNKNOWN
        elif isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("places holds integers, None or -1")
        v = int(v)
        if v == -1:
            v = AGGV_UNKNOWN
        if v < 0 or v > 0xFFFFFFFF:
            raise ValueError("places holds places of a pool's lanes, 0 .. 2^32 - 2, and None or -1 for an unknown lane")
        out[i] = v
    return out


def _dev_result(d_result, engine):
    if (str(getattr(d_result, "dtype", None)) not in ("torch.int32", "torch.uint32") or d_result.numel() < 1
            or not d_result.is_contiguous() or not _on_device(d_result, engine)):
        raise ValueError("d_result is one 32-bit integer on the engine's device")


def _on_device(t, engine):
    """the tensor lies on the engine's GPU"""
    dev = getattr(t, "device", None)
    return dev is not None and dev.type == "cuda" and (dev.index or 0) == int(getattr(engine, "device", 0) or 0)


def _dev_order(d_order, engine):
    """a list of places in device memory as the _device forms take it: a contiguous one-dimensional int32 / uint32 tensor
    on the engine's device (the address is handed to the kernel as it is) -> its length; ValueError otherwise"""
    if str(getattr(d_order, "dtype", None)) not in ("torch.int32", "torch.uint32"):
        raise ValueError("d_order holds 32-bit integer indices (torch.int32 or torch.uint32)")
    if d_order.dim() != 1 or not d_order.is_contiguous():
        raise ValueError("d_order is a contiguous one-dimensional tensor")
    if not _on_device(d_order, engine):
        raise ValueError("d_order lies on the engine's device")
    return int(d_order.numel())


def _dev_bytes(t, engine, name):
    """an output of a _device form: a contiguous uint8 tensor on the engine's device; ValueError otherwise"""
    if str(getattr(t, "dtype", None)) != "torch.uint8" or not t.is_contiguous() or not _on_device(t, engine):
        raise ValueError("%s is a contiguous uint8 tensor on the engine's device" % name)


class _LaneStore(_Handle):
    """what the two streaming objects share: the eight info words under the names of _fields, len() = the lanes held,
    reset()"""
    _fields = None

    def info(self):
        """the eight words of ssa_<_prefix>_info by the names of _fields (AGGREGATOR_FIELDS, AGGVERIFIER_FIELDS)"""
        out = (C.c_uint64 * 8)()
        self._call("info", self.handle, out)
        return dict(zip(self._fields, (int(v) for v in out)))

    def __len__(self):
        return self.info()["held"]

    def reset(self):
        """forget every lane and restart the counters; the memory stays"""
        self._call("reset", self.handle)


class Aggregator(_LaneStore):
    """ssa_aggregator handle (Engine.aggregator): the lanes admitted so far, on the device, in
    arrival order.  push() admits a batch on arrival; finish() gives the AggregateSignature of the first n_take held
    lanes -- what Engine.aggregate gives those lanes handed in alone -- and changes nothing; drop_front(), remove() and
    take() remove lanes in place and keep the rest of the pool; push(cache=) and push_keyed()
    admit through a key cache, and an object made with hold_keys=True keeps the admitted lanes' wire keys for keys() and
    take_block(); finish_select(), remove_indices() and take_select() do the same for lanes of
    the caller's choosing, in the caller's order.  Tied to its Engine like KeyCache; destroyed exactly once (close(), the end of
    a `with` block, or when the object goes away)."""
    _prefix, _fields = "aggregator", AGGREGATOR_FIELDS

    def __init__(self, engine, handle, hold_keys=False, hold_admission=False, index=False):
        super().__init__(engine, handle)
        self.hold_keys = bool(hold_keys)
        self.hold_admission = bool(hold_admission)
        self.index = bool(index)

    # ---- the leaf column and the leaf index
    def leaves(self, n=None):
        """the 32-byte leaves -- the ids -- of the first n held lanes (None: all) as uint8[n, 32], in arrival order.
        Changes no state; every aggregator has them."""
        held = self.info()["held"]
        k = held if n is None else int(n)
        out = np.full((max(min(k, held), 1), 32), 255, dtype=np.uint8)
        _check(_lib.ssa_aggregator_leaves(self.engine._ctx, self.handle, _n_take(n), _ptr(out)), "ssa_aggregator_leaves")
        return out[:min(k, held)].copy()

    def leaves_device(self, d_ids32, n=None):
        """device form: only enqueues; the 32 n bytes land in the uint8 tensor d_ids32 (any byte alignment), n as given
        or all lanes held.  Returns n."""
        k = self.info()["held"] if n is None else int(n)
        _dev_bytes(d_ids32, self.engine, "d_ids32")
        if d_ids32.numel() < 32 * k:
            raise ValueError("the leaves of %d lanes are %d bytes" % (k, 32 * k))
        _check(_lib.ssa_aggregator_leaves_device(self.engine._ctx, self.handle, k, d_ids32.data_ptr()),
               "ssa_aggregator_leaves_device")
        return k

    def leaves_select(self, order):
        """the leaves of the held lanes at the places order[0], order[1], ... in THAT order as uint8[m, 32]: the id
        column that goes beside finish_select(order).  A place may be named twice; an index that is not below the lanes
        held is refused by the device and raises as every SSA_ERR_ARG does."""
        order = _order_u32(order)
        m = int(order.size)
        out = np.full((max(m, 1), 32), 255, dtype=np.uint8)
        _check(_lib.ssa_aggregator_leaves_select(self.engine._ctx, self.handle, _ptr(order) if m else None, m, _ptr(out)),
               "ssa_aggregator_leaves_select")
        return out[:m].copy()

    def leaves_select_device(self, d_order, d_ids32, d_result):
        """device form: only enqueues.  d_order: m 32-bit indices on the engine's device; the 32 m bytes land in the
        uint8 tensor d_ids32 (any byte alignment); d_result (one int32 on the device) receives 0, or 1 for a list with
        an index out of range, whose output is zeroed.  Returns m."""
        m = _dev_order(d_order, self.engine)
        _dev_bytes(d_ids32, self.engine, "d_ids32")
        _dev_result(d_result, self.engine)
        if d_ids32.numel() < 32 * m:
            raise ValueError("the leaves of %d lanes are %d bytes" % (m, 32 * m))
        _check(_lib.ssa_aggregator_leaves_select_device(self.engine._ctx, self.handle, _addr(d_order), m,
                                                        d_ids32.data_ptr(), d_result.data_ptr()),
               "ssa_aggregator_leaves_select_device")
        return m

    def _need_index(self):
        if not self.index:
            raise ValueError("this aggregator was made without index=True (SSA_AGGR_HOLD_INDEX)")

    def index_sync(self):
        """brings the leaf index up to date with the lanes held; only enqueues.  A lookup does the same in front of its
        query: calling this right after a removal takes the rebuild off the block's critical path."""
        self._need_index()
        _check(_lib.ssa_aggregator_index_sync(self.engine._ctx, self.handle), "ssa_aggregator_index_sync")

    def lookup(self, ids):
        """ids: n 32-byte leaves (uint8[n, 32], or any buffer of 32 n bytes) -> (places uint32[n], n_unknown):
        places[i] is the LOWEST place of the pool whose leaf is ids[i], or AGGV_UNKNOWN; n_unknown counts the latter.
        The pair is what AggregateVerifier.push_mixed* takes.  ValueError, before any call, on a pool made without
        index=True or for ids whose size is no multiple of 32."""
        self._need_index()
        a = np.ascontiguousarray(np.frombuffer(ids, dtype=np.uint8) if isinstance(ids, (bytes, bytearray, memoryview))
                                 else np.asarray(ids, dtype=np.uint8)).reshape(-1)
        if a.size % 32:
            raise ValueError("ids are 32 bytes each")
        n = a.size // 32
        places = np.full(max(n, 1), AGGV_UNKNOWN, dtype=np.uint32)
        unknown = C.c_uint64(0)
        _check(_lib.ssa_aggregator_lookup(self.engine._ctx, self.handle, _ptr(a) if n else None, n, _ptr(places),
                                          C.byref(unknown)), "ssa_aggregator_lookup")
        return places[:n].copy(), int(unknown.value)

    def lookup_device(self, d_ids, d_places, d_count):
        """device form: only enqueues (the index is brought up to date in front of the query).  d_ids: a contiguous
        uint8 tensor of 32 n bytes on the engine's device, any byte alignment; d_places: a 32-bit integer tensor of at
        least n words; d_count: one 32-bit integer, the number of AGGV_UNKNOWN answers.  Both outputs stay on the
        device: d_places goes unread into AggregateVerifier.push_mixed*_device.  Returns n."""
        self._need_index()
        _dev_bytes(d_ids, self.engine, "d_ids")
        if d_ids.numel() % 32:
            raise ValueError("ids are 32 bytes each")
        n = int(d_ids.numel()) // 32
        if _dev_order(d_places, self.engine) < n:
            raise ValueError("the places of %d ids are %d words" % (n, n))
        _dev_result(d_count, self.engine)
        _check(_lib.ssa_aggregator_lookup_device(self.engine._ctx, self.handle, d_ids.data_ptr() if n else None, n,
                                                 d_places.data_ptr() if n else None, d_count.data_ptr()),
               "ssa_aggregator_lookup_device")
        return n

    def index_info(self):
        """the eight words of ssa_aggregator_index_info by the names of AGGREGATOR_INDEX_FIELDS.  Synchronises the
        engine's stream once: `overflowed` is a counter on the device."""
        self._need_index()
        out = (C.c_uint64 * 8)()
        _check(_lib.ssa_aggregator_index_info(self.engine._ctx, self.handle, out), "ssa_aggregator_index_info")
        return dict(zip(AGGREGATOR_INDEX_FIELDS, (int(v) for v in out)))

    def admission(self, n=None):
        """the admission classes (ADM_*) of the first n held lanes (None: all) as uint8[n], in arrival order: how the
        push that admitted each lane screened it.  Changes no state.  An object made without
        hold_admission raises."""
        held = self.info()["held"]
        k = held if n is None else int(n)
        out = np.full(max(min(k, held), 1), 255, dtype=np.uint8)
        _check(_lib.ssa_aggregator_admission(self.engine._ctx, self.handle, _n_take(n), _ptr(out)),
               "ssa_aggregator_admission")
        return out[:min(k, held)].copy()

    def admission_device(self, d_adm, n=None):
        """device form: only enqueues on the engine's stream; the n bytes land in the uint8 tensor d_adm, n as given or
        all lanes held.  Returns n."""
        k = self.info()["held"] if n is None else int(n)
        _dev_bytes(d_adm, self.engine, "d_adm")
        if d_adm.numel() < k:
            raise ValueError("the classes of %d lanes are %d bytes" % (k, k))
        _check(_lib.ssa_aggregator_admission_device(self.engine._ctx, self.handle, k, d_adm.data_ptr()),
               "ssa_aggregator_admission_device")
        return k

    def push(self, sigs, pks, msgs, pk_inf=None, screen=True, offsets=None, engine=None, cache=None):
        """a batch of signatures, keys and messages as Engine.aggregate_valid takes them -> (status uint8[n], n_kept):
        the lanes whose status is zero are appended in lane order.  screen=True: the statuses of
        Engine.verify_batch_screened on this batch alone; screen=False (SSA_AGGR_NO_SCREEN): 0 or MALFORMED by the checks
        of Engine.aggregate(check=False), for a producer that made the signatures itself.  A batch that does not fit
        what is left of the capacity raises and changes nothing.  engine: tests (a context other than the object's).
        cache: an AFFINE KeyCache -- the statuses, and the stats, of
        Engine.aggregate_valid_cached on this batch alone and the same cache: a lane whose key lies outside the subgroup
        is dropped with INVALID_PUBLIC_KEY.  Then returns (status, n_kept, stats uint64[12])."""
        eng = engine or self.engine
        n, batch, keep = eng._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        status = np.full(n, 255, dtype=np.uint8)
        n_kept = C.c_uint64(0)
        if cache is not None:
            if screen is not True:
                raise ValueError("a cached push always screens")
            stats = np.zeros(12, dtype=np.uint64)
            _check(_lib.ssa_aggregator_push_cached(eng._ctx, self.handle, cache.handle, *batch, _ptr(status) if n else None,
                                                   C.byref(n_kept), stats.ctypes.data), "ssa_aggregator_push_cached")
            return status, int(n_kept.value), stats
        _check(_lib.ssa_aggregator_push(eng._ctx, self.handle, *batch, 0 if screen else AGGR_NO_SCREEN,
                                        _ptr(status) if n else None, C.byref(n_kept)), "ssa_aggregator_push")
        return status, int(n_kept.value)

    def push_keyed(self, cache, keyed, msgs, offsets=None, engine=None):
        """n 130-byte KeyedSignature records pk(49) || sig(81) through a key cache made with wire=True (DESIGN.md
        section 31) -> (status uint8[n], n_kept, stats uint64[12]): status and stats are those of
        Engine.aggregate_valid_keyed_cached on this batch alone and the same cache; the lanes of status zero are appended
        in lane order, and an object made with hold_keys=True keeps their 49 key bytes.  cache=None raises as the
        library refuses it.  engine: tests."""
        eng = engine or self.engine
        kd = _np_u8(keyed, 130)
        n = kd.shape[0]
        m_, off, stride, mlen = eng._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        status = np.full(n, 255, dtype=np.uint8)
        stats = np.zeros(12, dtype=np.uint64)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_push_keyed_cached(
            eng._ctx, self.handle, None if cache is None else cache.handle, _ptr(kd) if n else None, _ptr(m_), _ptr(off),
            stride, mlen, n, _ptr(status) if n else None, C.byref(n_kept), stats.ctypes.data),
            "ssa_aggregator_push_keyed_cached")
        return status, int(n_kept.value), stats

    def push_cached_device(self, cache, d_sigs, d_pks, d_msgs, d_status=None, d_pk_inf=None, d_offsets=None, msg_len=None,
                           msg_stride=None, want_stats=True):
        """device form of push(cache=) over torch tensors on the engine's device, shaped as push_device takes them.
        Synchronises the stream as Engine.aggregate_valid_cached_device does -> (n_kept, stats uint64[12] or None)."""
        n = int(d_pks.shape[0])
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
        n_kept = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggregator_push_cached_device(
            self.engine._ctx, self.handle, cache.handle, _addr(d_sigs), _addr(d_pks), _addr(d_pk_inf), _addr(d_msgs),
            _addr(d_offsets), stride, mlen, n, _addr(d_status), C.byref(n_kept), stats.ctypes.data if want_stats else None),
            "ssa_aggregator_push_cached_device")
        return int(n_kept.value), stats

    def push_keyed_device(self, cache, d_keyed, d_msgs, d_status=None, d_offsets=None, msg_len=None, msg_stride=None,
                          want_stats=True):
        """device form of push_keyed: d_keyed an (n, 130) uint8 tensor on the engine's device -> (n_kept, stats uint64[12]
        or None).  Synchronises as push_cached_device."""
        n = int(d_keyed.shape[0])
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
        n_kept = C.c_uint64(0)
        stats = np.zeros(12, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggregator_push_keyed_cached_device(
            self.engine._ctx, self.handle, cache.handle, _addr(d_keyed), _addr(d_msgs), _addr(d_offsets), stride, mlen, n,
            _addr(d_status), C.byref(n_kept), stats.ctypes.data if want_stats else None),
            "ssa_aggregator_push_keyed_cached_device")
        return int(n_kept.value), stats

    def keys(self, n_take=None):
        """the 49-byte wire keys of the first n_take held lanes (None: all) as uint8[n, 49], in arrival order: the first
        49 bytes of each admitted record, verbatim.  Changes no state.  An object made without hold_keys raises."""
        held = self.info()["held"]
        n = held if n_take is None else int(n_take)
        out = np.full((max(min(n, held), 1), 49), 255, dtype=np.uint8)
        _check(_lib.ssa_aggregator_keys(self.engine._ctx, self.handle, _n_take(n_take), _ptr(out)), "ssa_aggregator_keys")
        return out[:min(n, held)].copy()

    def keys_device(self, d_keys49, n_take=None):
        """device form: only enqueues on the engine's stream; the 49 n bytes land in the uint8 tensor d_keys49 (any byte
        alignment), n = n_take or all lanes held.  Returns n."""
        n = self.info()["held"] if n_take is None else int(n_take)
        if d_keys49.numel() < 49 * n:
            raise ValueError("the keys of %d lanes are %d bytes" % (n, 49 * n))
        _check(_lib.ssa_aggregator_keys_device(self.engine._ctx, self.handle, n, d_keys49.data_ptr()),
               "ssa_aggregator_keys_device")
        return n

    def push_device(self, d_sigs, d_pks, d_msgs, d_status=None, d_pk_inf=None, d_offsets=None, msg_len=None,
                    msg_stride=None, screen=True):
        """device form over torch tensors on the engine's device: d_sigs (n, 81), d_pks (n, 96), d_msgs an (n, len) uint8
        tensor (or flat bytes with a uint64-valued d_offsets and msg_len left None); the statuses land in d_status
        (uint8[n]) when it is given.  Synchronises the stream (inside the screen, and for the kept count) -> n_kept."""
        n = int(d_pks.shape[0])
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_push_device(
            self.engine._ctx, self.handle, _addr(d_sigs), _addr(d_pks), _addr(d_pk_inf), _addr(d_msgs), _addr(d_offsets),
            stride, mlen, n, 0 if screen else AGGR_NO_SCREEN, _addr(d_status), C.byref(n_kept)),
            "ssa_aggregator_push_device")
        return int(n_kept.value)

    def finish_bytes(self, n_take=None):
        """the aggregate of the first n_take held lanes (None: all) as a uint8[49 n + 32] array"""
        held = self.info()["held"]
        n = held if n_take is None else int(n_take)
        agg = np.full(49 * min(n, held) + 32, 255, dtype=np.uint8)
        _check(_lib.ssa_aggregator_finish(self.engine._ctx, self.handle, _n_take(n_take), _ptr(agg)), "ssa_aggregator_finish")
        return agg

    def finish(self, n_take=None):
        """-> the AggregateSignature of the first n_take held lanes (None: all of them; the block-size limit of a
        producer whose pool exceeds the block).  Changes no state: it may be repeated, called with another n_take, and
        followed by more pushes.  n_take above the lanes held raises."""
        return AggregateSignature(self.finish_bytes(n_take).tobytes())

    def finish_device(self, d_agg, n_take=None):
        """device form: only enqueues on the engine's stream; the 49 n + 32 bytes land in the uint8 tensor d_agg (any
        byte alignment), n = n_take or all lanes held.  Returns n."""
        n = self.info()["held"] if n_take is None else int(n_take)
        if d_agg.numel() < 49 * n + 32:
            raise ValueError("an aggregate of %d signatures is %d bytes" % (n, 49 * n + 32))
        _check(_lib.ssa_aggregator_finish_device(self.engine._ctx, self.handle, n, d_agg.data_ptr()),
               "ssa_aggregator_finish_device")
        return n

    def drop_front(self, n=None, engine=None):
        """removes the first n held lanes in place (None: all of them): the object is then what
        it would be had it admitted the remaining lanes alone, in their order; the counters but `held` and `blocks` do
        not move.  Only enqueues.  n above the lanes held raises and changes nothing.  engine: tests."""
        _check(_lib.ssa_aggregator_drop_front((engine or self.engine)._ctx, self.handle, _n_take(n)),
               "ssa_aggregator_drop_front")

    def remove(self, drop, engine=None):
        """drop: one byte per held lane; lane i is removed iff drop[i] != 0 (the status vector of a screen can be handed
        in as it is) -> the number of lanes kept.  The kept lanes stay in their order, as if they alone had been
        admitted.  Another length raises and changes nothing.  engine: tests."""
        drop = np.ascontiguousarray(drop, dtype=np.uint8).reshape(-1)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_remove((engine or self.engine)._ctx, self.handle, _ptr(drop) if drop.size else None,
                                          drop.size, C.byref(n_kept)), "ssa_aggregator_remove")
        return int(n_kept.value)

    def remove_device(self, d_drop):
        """device form of remove over a uint8 torch tensor on the engine's device (any byte alignment), one byte per held
        lane.  Synchronises the stream once, for the kept count -> that count."""
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_remove_device(self.engine._ctx, self.handle, _addr(d_drop), int(d_drop.numel()),
                                                 C.byref(n_kept)), "ssa_aggregator_remove_device")
        return int(n_kept.value)

    def finish_select_bytes(self, order, keys=False):
        """the aggregate of the held lanes at the places order[0], order[1], ... in that order, as uint8[49 m + 32]; with
        keys=True (an object made with hold_keys=True) -> (that, their wire keys uint8[m, 49])"""
        order = _order_u32(order)
        m = int(order.size)
        agg = np.full(49 * m + 32, 255, dtype=np.uint8)
        k49 = np.full((max(m, 1), 49), 255, dtype=np.uint8) if keys else None
        _check(_lib.ssa_aggregator_finish_select(self.engine._ctx, self.handle, _ptr(order) if m else None, m, _ptr(agg),
                                                 _ptr(k49)), "ssa_aggregator_finish_select")
        return (agg, k49[:m].copy()) if keys else agg

    def finish_select(self, order, keys=False):
        """-> the AggregateSignature of the held lanes order[0], order[1], ... (distinct places below the lanes held, any
        integer sequence or array) in THAT order: what Engine.aggregate gives those lanes handed in alone (DESIGN.md
        section 32).  Changes no state, like finish.  keys=True: -> (aggregate, keys uint8[m, 49]), the block body's key
        column in the same order.  Indices that do not fit 32 bits raise ValueError here; an index out of range or named
        twice is refused by the device and raises as every SSA_ERR_ARG does."""
        out = self.finish_select_bytes(order, keys)
        return (AggregateSignature(out[0].tobytes()), out[1]) if keys else AggregateSignature(out.tobytes())

    def finish_select_device(self, d_order, d_agg, d_result, d_keys49=None):
        """device form: only enqueues on the engine's stream.  d_order: an int32 / uint32-valued tensor of m indices on
        the engine's device (4-byte aligned); the 49 m + 32 bytes land in the uint8 tensor d_agg, the 49 m key bytes in
        d_keys49 when it is given (both at any byte alignment), and d_result (one int32 on the device) receives 0 for a
        valid list, 1 for a refused one -- whose outputs are zeroed.  Returns m."""
        m = _dev_order(d_order, self.engine)
        _dev_bytes(d_agg, self.engine, "d_agg")
        if d_keys49 is not None:
            _dev_bytes(d_keys49, self.engine, "d_keys49")
        if (str(d_result.dtype) not in ("torch.int32", "torch.uint32") or d_result.numel() < 1 or not d_result.is_contiguous()
                or not _on_device(d_result, self.engine)):
            raise ValueError("d_result is one 32-bit integer on the engine's device")
        if d_agg.numel() < 49 * m + 32 or (d_keys49 is not None and d_keys49.numel() < 49 * m):
            raise ValueError("a selection of %d lanes is %d bytes and %d bytes of keys" % (m, 49 * m + 32, 49 * m))
        _check(_lib.ssa_aggregator_finish_select_device(
            self.engine._ctx, self.handle, _addr(d_order), m, d_agg.data_ptr(),
            None if d_keys49 is None else d_keys49.data_ptr(), d_result.data_ptr()), "ssa_aggregator_finish_select_device")
        return m

    def remove_indices(self, order, engine=None):
        """remove() with a list in place of a mask: the held lanes at the places named in `order` (distinct, below the
        lanes held, in any order) leave the object, the rest stays in arrival order -> the number of lanes kept.  An
        invalid list raises and changes nothing.  engine: tests."""
        order = _order_u32(order)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_remove_indices((engine or self.engine)._ctx, self.handle,
                                                  _ptr(order) if order.size else None, int(order.size), C.byref(n_kept)),
               "ssa_aggregator_remove_indices")
        return int(n_kept.value)

    def remove_indices_device(self, d_order):
        """device form of remove_indices over a 32-bit integer tensor on the engine's device.  Synchronises the stream
        once, as remove_device does -> the number of lanes kept."""
        m = _dev_order(d_order, self.engine)
        n_kept = C.c_uint64(0)
        _check(_lib.ssa_aggregator_remove_indices_device(self.engine._ctx, self.handle, _addr(d_order), m,
                                                         C.byref(n_kept)), "ssa_aggregator_remove_indices_device")
        return int(n_kept.value)

    def take_select(self, order):
        """finish_select(order) -- with the keys when the object holds them -- then remove_indices(order): the chosen
        lanes leave as a block body, the rest stays, in arrival order, for the next slot.  -> AggregateSignature, or
        (AggregateSignature, keys uint8[m, 49]) from an object made with hold_keys=True"""
        order = _order_u32(order)
        out = self.finish_select(order, keys=self.hold_keys)
        self.remove_indices(order)
        return out

    def take(self, n_take=None):
        """finish(n_take), then drop_front of the same lanes: the AggregateSignature of the first n_take held lanes
        (None: all), which leave the object; the rest stays for the next block"""
        n = self.info()["held"] if n_take is None else int(n_take)
        agg = self.finish(n)
        self.drop_front(n)
        return agg

    def take_block(self, n_take=None):
        """take() of an object made with hold_keys=True -> (AggregateSignature, keys uint8[n, 49]): the aggregate and the
        key column of the block body; the lanes leave the object, the rest stays for the next block"""
        n = self.info()["held"] if n_take is None else int(n_take)
        agg, keys = self.finish(n), self.keys(n)
        self.drop_front(n)
        return agg, keys


class AggregateVerifier(_LaneStore):
    """ssa_aggverifier handle (Engine.aggregate_verifier): the lanes of a block body pushed so
    far, on the device, in arrival order.  push() does the position-independent work of Engine.verify_aggregate on
    arrival; finish(e_agg) gives the status Engine.verify_aggregate gives the first n_take held lanes handed in at once
    with that e_agg -- and changes nothing.  Tied to its Engine like KeyCache; destroyed exactly once (close(), the end
    of a `with` block, or when the object goes away)."""
    _prefix, _fields = "aggverifier", AGGVERIFIER_FIELDS

    def cached_lanes(self):
        """the lanes pushed through a key cache since create or reset (word [5] of ssa_aggverifier_info)"""
        return self.info()["reserved"]

    def push(self, rs49, pks, msgs, offsets=None, pk_inf=None, engine=None, cache=None):
        """n R's (n x 49 bytes, the aggregate's wire layout), keys and messages as Engine.verify_aggregate takes them:
        ALL n lanes are appended (a lane that fails a check makes every finish that takes it MALFORMED).  A batch that
        does not fit what is left of the capacity raises and changes nothing.  engine: tests (a context other than the
        object's).  Returns n.
        cache: an AFFINE KeyCache -- every distinct key is checked once, subgroup check included,
        and a finish that takes a lane whose key is outside the subgroup answers INVALID_PUBLIC_KEY.  Then returns
        (n, stats uint64[8]): words [0..5] of Engine.verify_aggregates_cached, [6] = [7] = 0.  Lanes pushed without a
        cache are "not checked" and never answer so; both kinds may be mixed in one object."""
        eng = engine or self.engine
        n, batch, keep = eng._agg_batch(rs49, 49, pks, msgs, offsets, pk_inf)
        if cache is None:
            _check(_lib.ssa_aggverifier_push(eng._ctx, self.handle, *batch), "ssa_aggverifier_push")
            return n
        if cache.wire:
            raise ValueError("push takes affine keys and an affine key cache: push_wire takes the 49-byte keys")
        stats = np.zeros(8, dtype=np.uint64)
        _check(_lib.ssa_aggverifier_push_cached(eng._ctx, self.handle, cache.handle, *batch, stats.ctypes.data),
               "ssa_aggverifier_push_cached")
        return n, stats

    def push_wire(self, rs49, pks49, msgs, offsets=None, cache=None, engine=None):
        """push with n dense 49-byte keys through a key cache made with wire=True (required): a key is decompressed
        once, when the cache first sees it.  -> (n, stats uint64[8]) as push(cache=...)."""
        if cache is None or not cache.wire:
            raise ValueError("push_wire needs a key cache made with wire=True")
        eng = engine or self.engine
        keys = _np_u8(pks49, 49)
        n = keys.shape[0]
        lead = _np_u8(rs49).reshape(-1)
        if lead.size not in (49 * n, 49 * n + 32):
            raise MalformedInput("We should have the same number of signatures than public keys")
        m, off, stride, mlen = eng._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        stats = np.zeros(8, dtype=np.uint64)
        _check(_lib.ssa_aggverifier_push_cached_wire(eng._ctx, self.handle, cache.handle, _ptr(lead), _ptr(keys) if n else None,
                                                     _ptr(m), _ptr(off), stride, mlen, n, stats.ctypes.data),
               "ssa_aggverifier_push_cached_wire")
        return n, stats

    def push_aggregate(self, agg, pks, msgs, offsets=None, pk_inf=None, cache=None):
        """the R's of an AggregateSignature (or its 49 n + 32 bytes) with their keys and messages; e_agg is not kept:
        hand it to finish().  Returns n; with a cache (affine keys and an affine cache, or 49-byte keys and a wire
        cache) what push(cache=...) / push_wire return."""
        b = np.frombuffer(agg.bytes if isinstance(agg, AggregateSignature) else bytes(agg), np.uint8)
        if cache is not None and cache.wire:
            if pk_inf is not None:
                raise ValueError("pk_inf does not go with wire keys: the 49 bytes carry the identity flag")
            return self.push_wire(b[:b.size - 32], pks, msgs, offsets=offsets, cache=cache)
        return self.push(b[:b.size - 32], pks, msgs, offsets=offsets, pk_inf=pk_inf, cache=cache)

    def _push_device_args(self, d_keys, d_msgs, d_offsets, msg_len, msg_stride, width):
        have = 0 if d_keys is None else d_keys.numel() * d_keys.element_size()
        if have % width:
            raise ValueError("the keys are %d bytes each" % width)
        return (have // width,) + _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride, no_msgs_ok=True)

    def push_device(self, d_rs49, d_pks, d_msgs, d_pk_inf=None, d_offsets=None, msg_len=None, msg_stride=None, cache=None,
                    want_stats=True):
        """device form over torch tensors on the engine's device: d_rs49 (n, 49), d_pks (n, 96), d_msgs an (n, len)
        uint8 tensor (or flat bytes with a uint64-valued d_offsets and msg_len left None).  Only enqueues.  Returns n.
        cache: an affine KeyCache, as push().  Then the call synchronises the stream once per slice of SSA_LANE_SLICE
        lanes (the key dedup's read-back), with want_stats once more at the end, and returns (n, stats or None)."""
        if cache is None:
            n = int(d_pks.shape[0])
            stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride)
            _check(_lib.ssa_aggverifier_push_device(
                self.engine._ctx, self.handle, _addr(d_rs49), _addr(d_pks), _addr(d_pk_inf), _addr(d_msgs), _addr(d_offsets),
                stride, mlen, n), "ssa_aggverifier_push_device")
            return n
        if cache.wire:
            raise ValueError("push_device takes affine keys and an affine key cache: push_wire_device takes the 49-byte keys")
        n, stride, mlen = self._push_device_args(d_pks, d_msgs, d_offsets, msg_len, msg_stride, 96)
        stats = np.zeros(8, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggverifier_push_cached_device(
            self.engine._ctx, self.handle, cache.handle, _addr(d_rs49), _addr(d_pks), _addr(d_pk_inf), _addr(d_msgs),
            _addr(d_offsets), stride, mlen, n, stats.ctypes.data if want_stats else None), "ssa_aggverifier_push_cached_device")
        return n, stats

    def push_wire_device(self, d_rs49, d_pks49, d_msgs, d_offsets=None, msg_len=None, msg_stride=None, cache=None,
                         want_stats=True):
        """device form of push_wire: d_pks49 holds n x 49 bytes -> (n, stats or None).  Synchronises as
        push_device(cache=...)."""
        if cache is None or not cache.wire:
            raise ValueError("push_wire_device needs a key cache made with wire=True")
        n, stride, mlen = self._push_device_args(d_pks49, d_msgs, d_offsets, msg_len, msg_stride, 49)
        stats = np.zeros(8, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggverifier_push_cached_wire_device(
            self.engine._ctx, self.handle, cache.handle, _addr(d_rs49), _addr(d_pks49), _addr(d_msgs), _addr(d_offsets), stride,
            mlen, n, stats.ctypes.data if want_stats else None), "ssa_aggverifier_push_cached_wire_device")
        return n, stats

    def finish(self, e_agg, n_take=None):
        """-> the int status of the first n_take held lanes (None: all) under e_agg (32 bytes): OK, INVALID_SIGNATURE or
        MALFORMED, what Engine.verify_aggregate returns for those lanes and that scalar.  Changes no state: it may be
        repeated, take prefixes, and be followed by more pushes.  n_take above the lanes held raises."""
        e = _np_u8(e_agg).reshape(-1)
        if e.size != 32:
            raise ValueError("e_agg is 32 bytes")
        return _check(_lib.ssa_aggverifier_finish(self.engine._ctx, self.handle, _ptr(e), _n_take(n_take)),
                      "ssa_aggverifier_finish")

    def finish_device(self, d_e_agg, d_verdict, n_take=None):
        """device form: only enqueues on the engine's stream; d_e_agg a uint8 tensor of 32 bytes, the status lands in the
        first element of the int32 / uint32 tensor (view) d_verdict"""
        _check(_lib.ssa_aggverifier_finish_device(self.engine._ctx, self.handle, d_e_agg.data_ptr(), _n_take(n_take),
                                                  d_verdict.data_ptr()), "ssa_aggverifier_finish_device")

    def record(self, n_take=None):
        """tests: the 24-word record finish compares with [e_agg]G (ssa_debug_aggverifier_record) as uint64[24]"""
        import torch
        d_rec = torch.zeros(MSM_PARTIAL_WORDS, dtype=torch.int64, device="cuda:%d" % self.engine.device)
        torch.cuda.synchronize(d_rec.device)      # (the engine's stream is not torch's)
        _check(_lib.ssa_debug_aggverifier_record(self.engine._ctx, self.handle, _n_take(n_take), d_rec.data_ptr()),
               "ssa_debug_aggverifier_record")
        self.engine.sync()
        return d_rec.cpu().numpy().view(np.uint64)

    # ---- a block against the pool
    def _mixed_cached_check(self, aggregator, cache, require, wire):
        """what the host can see of a mixed push through a key cache, before any call: ValueError"""
        require = _require_class(require)
        if cache is None:
            if require:
                raise ValueError("require > 0 goes with a key cache: the class is enforced by the cached mixed push")
            return 0
        if bool(cache.wire) != wire:
            raise ValueError("push_mixed takes affine keys and an affine key cache, push_mixed_wire 49-byte keys and a "
                             "cache made with wire=True")
        if require and not getattr(aggregator, "hold_admission", False):
            raise ValueError("require > 0 needs an Aggregator made with hold_admission=True")
        return require

    def push_mixed(self, aggregator, places, rs49, pks, msgs, offsets=None, pk_inf=None, engine=None, cache=None,
                   require=0):
        """n lanes of a block, most of them held by `aggregator` (an Aggregator of the same Engine) already: places[i]
        is the pool's place of lane i, or None / -1 for a lane the pool does not hold.  The u unknown lanes come with
        the call, side by side in block order (rs49, pks, msgs, pk_inf as push() takes them) and are treated as
        push() treats them; a known lane takes leaf and scalar from the pool, copied.  finish() then answers as for
        the block with every known lane replaced by what the pool admitted it with -- PROVIDED the pool's scalar of
        every known lane satisfies its verification equation: name only lanes admitted by a screened or cached push.
        An invalid list (a place not held, a count of unknown lanes other than u) raises and changes nothing.
        engine: tests.  Returns n.
        cache: an AFFINE KeyCache -- the unknown lanes go through it as push(cache=) sends
        them, and a known lane whose admission class in the pool (Aggregator.admission) is below `require` (0, 1 or 2;
        above 0 the pool must be made with hold_admission=True) is refused: the call raises and changes nothing.  With
        require=2 on lanes the pool admitted through a cache, finish() answers what Engine.verify_aggregates_cached
        answers for the whole block, with nothing owed by the caller.  Then returns (n, stats uint64[8])."""
        require = self._mixed_cached_check(aggregator, cache, require, False)
        places = _places_u32(places)
        n = int(places.size)
        eng = engine or self.engine
        u, batch, keep = eng._agg_batch(rs49, 49, pks, msgs, offsets, pk_inf)
        ag = aggregator.handle if aggregator is not None else None
        if cache is not None:
            stats = np.zeros(8, dtype=np.uint64)
            _check(_lib.ssa_aggverifier_push_mixed_cached(eng._ctx, self.handle, ag, cache.handle, _ptr(places) if n else None,
                                                          n, *batch, require, stats.ctypes.data),
                   "ssa_aggverifier_push_mixed_cached")
            return n, stats
        _check(_lib.ssa_aggverifier_push_mixed(eng._ctx, self.handle, ag, _ptr(places) if n else None, n, *batch),
               "ssa_aggverifier_push_mixed")
        return n

    def push_mixed_wire(self, aggregator, places, rs49, pks49, msgs, offsets=None, cache=None, require=0, engine=None):
        """push_mixed with the u unknown lanes' keys as dense 49-byte wire keys through a key cache made with wire=True
        (required): what push_wire does for the unknown lanes, `require` as in push_mixed.  -> (n, stats uint64[8])."""
        if cache is None:
            raise ValueError("push_mixed_wire needs a key cache made with wire=True")
        require = self._mixed_cached_check(aggregator, cache, require, True)
        places = _places_u32(places)
        n = int(places.size)
        eng = engine or self.engine
        keys = _np_u8(pks49, 49)
        u = keys.shape[0]
        lead = _np_u8(rs49).reshape(-1)
        if lead.size != 49 * u:
            raise MalformedInput("We should have the same number of signatures than public keys")
        m, off, stride, mlen = eng._msg_args(msgs, offsets, u) if u else (None, None, 0, 0)
        stats = np.zeros(8, dtype=np.uint64)
        _check(_lib.ssa_aggverifier_push_mixed_cached_wire(
            eng._ctx, self.handle, aggregator.handle if aggregator is not None else None, cache.handle,
            _ptr(places) if n else None, n, _ptr(lead) if u else None, _ptr(keys) if u else None, _ptr(m), _ptr(off), stride,
            mlen, u, require, stats.ctypes.data), "ssa_aggverifier_push_mixed_cached_wire")
        return n, stats

    def push_known(self, aggregator, places, engine=None, cache=None, require=0):
        """push_mixed without unknown lanes: every lane of the block is held by the pool.  Returns n.
        require > 0 (with the cache the object's other lanes go through, affine or wire: no key is sent to it) routes
        through the cached mixed push with u = 0, which enforces the class and makes the object keyed; require == 0
        is the plain call, whatever `cache` is."""
        require = _require_class(require)
        if require:
            if cache is None:
                raise ValueError("require > 0 goes with a key cache: the class is enforced by the cached mixed push")
            if cache.wire:
                return self.push_mixed_wire(aggregator, places, np.zeros(0, np.uint8), np.zeros((0, 49), np.uint8), None,
                                            cache=cache, require=require, engine=engine)[0]
            return self.push_mixed(aggregator, places, np.zeros(0, np.uint8), np.zeros((0, 96), np.uint8), None,
                                   engine=engine, cache=cache, require=require)[0]
        places = _places_u32(places)
        n = int(places.size)
        _check(_lib.ssa_aggverifier_push_known((engine or self.engine)._ctx, self.handle,
                                               aggregator.handle if aggregator is not None else None,
                                               _ptr(places) if n else None, n), "ssa_aggverifier_push_known")
        return n

    def push_mixed_device(self, aggregator, d_places, d_result, d_rs49, d_pks, d_msgs, d_pk_inf=None, d_offsets=None,
                          msg_len=None, msg_stride=None, cache=None, require=0, want_stats=True):
        """device form: only enqueues on the engine's stream.  d_places: an int32 / uint32-valued tensor of n places on
        the engine's device (AGGV_UNKNOWN, or -1 as int32, for an unknown lane); the u unknown lanes as push_device
        takes them (u = the rows of d_pks; None: no unknown lane).  d_result (one int32 on the device) receives 0 for a
        valid list, 1 for a refused one, whose lanes are held as failed: every finish that reaches one answers MALFORMED.
        Returns n.
        cache, require: as push_mixed (an affine cache).  Then the call is NOT enqueue-only -- it synchronises the
        stream once per slice of the unknown keys, as push_device(cache=) does -- d_result gets bit 0 for an invalid
        list and bit 1 for a known lane below the required class, and the call returns (n, stats or None)."""
        require = self._mixed_cached_check(aggregator, cache, require, False)
        n = _dev_order(d_places, self.engine)
        _dev_result(d_result, self.engine)
        u = 0 if d_pks is None else int(d_pks.shape[0])
        stride, mlen = _dev_msg_shape(d_msgs, d_offsets, msg_len, msg_stride, no_msgs_ok=True) if u else (0, 0)
        if cache is not None:
            stats = np.zeros(8, dtype=np.uint64) if want_stats else None
            _check(_lib.ssa_aggverifier_push_mixed_cached_device(
                self.engine._ctx, self.handle, aggregator.handle, cache.handle, _addr(d_places), n, _addr(d_rs49),
                _addr(d_pks), _addr(d_pk_inf), _addr(d_msgs), _addr(d_offsets), stride, mlen, u, require,
                d_result.data_ptr(), stats.ctypes.data if want_stats else None), "ssa_aggverifier_push_mixed_cached_device")
            return n, stats
        _check(_lib.ssa_aggverifier_push_mixed_device(
            self.engine._ctx, self.handle, aggregator.handle, _addr(d_places), n, _addr(d_rs49), _addr(d_pks), _addr(d_pk_inf),
            _addr(d_msgs), _addr(d_offsets), stride, mlen, u, d_result.data_ptr()), "ssa_aggverifier_push_mixed_device")
        return n

    def push_mixed_wire_device(self, aggregator, d_places, d_result, d_rs49, d_pks49, d_msgs, d_offsets=None, msg_len=None,
                               msg_stride=None, cache=None, require=0, want_stats=True):
        """device form of push_mixed_wire: d_pks49 holds u x 49 bytes (None: no unknown lane) -> (n, stats or None).
        Synchronises and reports as push_mixed_device(cache=...)."""
        if cache is None:
            raise ValueError("push_mixed_wire_device needs a key cache made with wire=True")
        require = self._mixed_cached_check(aggregator, cache, require, True)
        n = _dev_order(d_places, self.engine)
        _dev_result(d_result, self.engine)
        u, stride, mlen = self._push_device_args(d_pks49, d_msgs, d_offsets, msg_len, msg_stride, 49)
        stats = np.zeros(8, dtype=np.uint64) if want_stats else None
        _check(_lib.ssa_aggverifier_push_mixed_cached_wire_device(
            self.engine._ctx, self.handle, aggregator.handle, cache.handle, _addr(d_places), n, _addr(d_rs49), _addr(d_pks49),
            _addr(d_msgs), _addr(d_offsets), stride, mlen, u, require, d_result.data_ptr(),
            stats.ctypes.data if want_stats else None), "ssa_aggverifier_push_mixed_cached_wire_device")
        return n, stats

    def push_known_device(self, aggregator, d_places, d_result):
        """device form of push_known.  Returns n."""
        n = _dev_order(d_places, self.engine)
        _dev_result(d_result, self.engine)
        _check(_lib.ssa_aggverifier_push_known_device(self.engine._ctx, self.handle, aggregator.handle, _addr(d_places), n,
                                                      d_result.data_ptr()), "ssa_aggverifier_push_known_device")
        return n

    def known_sum(self, n_take=None):
        """tests: S = sum a_i s_i mod q over the known lanes of the first n_take held lanes (None: all) as a Python
        integer (ssa_debug_aggverifier_known_sum); 0 without a known lane"""
        import torch
        d_s = torch.zeros(32, dtype=torch.uint8, device="cuda:%d" % self.engine.device)
        torch.cuda.synchronize(d_s.device)      # (the engine's stream is not torch's)
        _check(_lib.ssa_debug_aggverifier_known_sum(self.engine._ctx, self.handle, _n_take(n_take), d_s.data_ptr()),
               "ssa_debug_aggverifier_known_sum")
        self.engine.sync()
        return int.from_bytes(d_s.cpu().numpy().tobytes(), "little")


class SignerSet:
    """ssa_signer_set handle: m key pairs held on the device, signing by index (KeyPair::sign for many messages).  Tied
    to its Engine like KeySet; destroyed exactly once (close(), or when the object goes away), which zeroes the secret
    keys on the device."""

    def __init__(self, engine, handle, m, public_keys=None):
        self.engine = engine      # keeps the context alive
        self.handle = handle
        self.m = int(m)
        self.public_keys = public_keys

    @classmethod
    def from_key_pairs(cls, key_pairs, engine=None):
        eng = engine or default_engine()
        sks = np.frombuffer(b"".join(kp.private_key.bytes for kp in key_pairs), np.uint8).reshape(-1, 32)
        ss = eng.signer_set_create(sks)
        ss.public_keys = [kp.public_key for kp in key_pairs]
        return ss

    @classmethod
    def generate(cls, m, engine=None):
        """KeyPair::new(rng) (src/keypair.rs:57-65) for m key pairs, the secret keys drawn on the device"""
        return (engine or default_engine()).signer_set_generate(m)

    def secret_keys(self):
        """KeyPair::to_bytes for every key pair -> uint8[m, 32]: the one call that brings the keys to the host"""
        return self.engine.signer_set_secret_keys(self)

    def sign(self, key_idx, messages, rng, constant_time=True, keyed=False):
        """KeyPair::sign (src/signature.rs:114-129) of messages[i] by key pair key_idx[i], nonces drawn as KeyPair
        draws them -> [Signature], or [KeyedSignature] (sign_and_bind_pkey, :132-156) with keyed=True.
        rng=DEVICE_RNG draws the nonces on the device."""
        idx = [int(k) for k in key_idx]
        if len(idx) != len(messages):
            raise ValueError("one key index per message")
        flat, off = pack_messages(messages)
        if rng is DEVICE_RNG:
            out = self.engine.sign_many_indexed_rng(self, np.array(idx, dtype=np.uint32), flat, offsets=off,
                                                    constant_time=constant_time, keyed=keyed)
        else:
            nonces = np.frombuffer(b"".join(KeyPair._nonce(None, rng) for _ in idx), np.uint8).reshape(-1, 32)
            out = self.engine.sign_many_indexed(self, np.array(idx, dtype=np.uint32), nonces, flat, offsets=off,
                                                constant_time=constant_time, keyed=keyed)
        if not keyed:
            return [Signature(r.tobytes()) for r in out]
        pub = self.public_keys
        if pub is None:
            pks, _ = self.engine.signer_set_public_keys(self)
            pub = self.public_keys = [PublicKey(p.tobytes()) for p in pks]
        return [KeyedSignature(pub[k], Signature(r[49:].tobytes())) for k, r in zip(idx, out)]

    def close(self):
        if self.handle:
            _lib.ssa_signer_set_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiEngine:
    """Several GPUs of one node from a single process (ssa_multi_*): contiguous shards, one context
    and one host thread per device, no collective."""

    def __init__(self, devices, params=None):
        self._m = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        blob = (C.c_uint8 * len(params)).from_buffer_copy(bytes(params)) if params is not None else None
        _check(_lib.ssa_multi_create(C.byref(self._m), devs, len(devices), blob, len(params) if params else 0),
               "ssa_multi_create")

    def close(self):
        if self._m:
            _lib.ssa_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_many(self, sigs, pks, msgs, offsets=None, check_torsion=True, pk_inf=None):
        sigs, pks = _np_u8(sigs, 81), _np_u8(pks, 96)
        n = sigs.shape[0]
        m = _np_u8(msgs)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        stride = mlen = 0 if off is not None else m.shape[1]
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        _check(_lib.ssa_multi_verify_many(self._m, _ptr(sigs), _ptr(pks), _ptr(inf), _ptr(m), _ptr(off), stride, mlen,
                                          n, FLAG_CHECK_TORSION if check_torsion else 0, _ptr(status),
                                          C.byref(nfail)), "ssa_multi_verify_many")
        return status, int(nfail.value)


    def verify_batch_msm(self, sigs, pks, msgs, offsets=None, coeffs=None, pk_inf=None):
        """verify_batch as the reference runs it, the batch sharded over the devices (one status)."""
        sigs, pks = _np_u8(sigs, 81), _np_u8(pks, 96)
        n = sigs.shape[0]
        m = _np_u8(msgs)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        stride = mlen = 0 if off is not None else m.shape[1]
        inf = _np_u8(pk_inf) if pk_inf is not None else None
        c = _np_u8(coeffs, 32) if coeffs is not None else None
        return _check(_lib.ssa_multi_verify_batch_msm(self._m, _ptr(sigs), _ptr(pks), _ptr(inf), _ptr(m), _ptr(off),
                                                      stride, mlen, n, _ptr(c)), "ssa_multi_verify_batch_msm")


    # half-aggregation with the blocks of the transcript dealt to the devices
    _msg_args = Engine._msg_args
    _agg_batch = Engine._agg_batch

    def aggregate(self, sigs, pks, msgs, offsets=None, pk_inf=None, check=False):
        """Engine.aggregate over the devices: the same (status, aggregate, per-lane status, n_fail), the same bytes"""
        n, batch, keep = self._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
        agg = np.full(49 * n + 32, 255, dtype=np.uint8)
        status = np.full(n, 255, dtype=np.uint8)
        nfail = C.c_uint64(0)
        st = _check(_lib.ssa_multi_aggregate_many(self._m, *batch, AGG_CHECK if check else 0, _ptr(agg),
                                                  _ptr(status) if n else None, C.byref(nfail)), "ssa_multi_aggregate_many")
        return st, agg, status, int(nfail.value)

    def verify_aggregate(self, agg, pks, msgs, offsets=None, pk_inf=None):
        """Engine.verify_aggregate over the devices -> status"""
        n, batch, keep = self._agg_batch(agg, 49, pks, msgs, offsets, pk_inf)
        if keep[0].size != 49 * n + 32:
            raise MalformedInput("an aggregate of n signatures is 49 n + 32 bytes")
        return _check(_lib.ssa_multi_verify_aggregate(self._m, *batch), "ssa_multi_verify_aggregate")

    aggregate_sliced, verify_aggregate_sliced = aggregate, verify_aggregate     # (its shards are sliced as they need)


_default_engine = None


def debug_tail_plan(waves, n, check_torsion=False, pieces=5, gens=1, uniform=False, min_main=0):
    """host logic of ssa_k_verify's end game (no device needed): the launch plan for n lanes with `waves` resident waves.
    Returns a dict: n_pieces, tail_groups, main_blocks, grid_blocks, pieces = [(pass, first, last, lo, hi)], whole"""
    out = np.zeros(14, dtype=np.uint32)
    flags = 1 if check_torsion else 0            # SSA_FLAG_CHECK_TORSION
    _check(_lib.ssa_debug_tail_plan(int(waves), int(pieces), int(gens), int(bool(uniform)), int(min_main), int(n), flags,
                                    out.ctypes.data), "ssa_debug_tail_plan")

    def dec(d):
        d = int(d)
        return (d & 1, bool(d & 2), bool(d & 4), (d >> 8) & 0xff, (d >> 16) & 0xff)
    return {"n_pieces": int(out[0]), "tail_groups": int(out[1]), "main_blocks": int(out[2]), "grid_blocks": int(out[3]),
            "pieces": [dec(out[4 + k]) for k in range(int(out[0]))], "whole": [dec(out[12]), dec(out[13])]}


def debug_split_plan(n, split_frac, split_min=0, check_torsion=False, force_lane=False, coop_max_n=7680,
                     coop_max_n_torsion=10496, twin=True):
    """host logic of the one-slice split (no device needed): (nA, nB) for a call of n lanes; nB == 0: not split"""
    out = np.zeros(2, dtype=np.uint64)
    flags = (FLAG_CHECK_TORSION if check_torsion else 0) | (FLAG_FORCE_LANE if force_lane else 0)
    _check(_lib.ssa_debug_split_plan(int(n), flags, int(split_min), int(split_frac), int(coop_max_n),
                                     int(coop_max_n_torsion), int(bool(twin)), out.ctypes.data), "ssa_debug_split_plan")
    return int(out[0]), int(out[1])


def debug_screen_plan(n, coeff_bytes=0):
    """host logic of the screened form (no device needed): its plan for n signatures at the default slice size"""
    out = np.zeros(8, dtype=np.uint64)
    _check(_lib.ssa_debug_screen_plan(int(n), int(coeff_bytes), out.ctypes.data), "ssa_debug_screen_plan")
    keys = ("segments", "segment_lanes", "window_bits", "windows", "r_windows", "buckets_per_window", "slices",
            "total_segments")
    return {k: int(v) for k, v in zip(keys, out)}


def debug_aggregates_plan(counts, msm_slice=1 << 23, small_max=3072):
    """host logic of verify_aggregates (no device needed): the plan of a call from its counts -> lanes, groups (one dict
    each) and the tree's passes (lists of (first node, nodes, slot, n_j of a top workgroup or 0)); None when refused"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts.size else None
    need = _lib.ssa_debug_aggregates_plan(cp, counts.size, int(msm_slice), int(small_max), None, 0)
    if need < 0:
        return None
    out = np.zeros(need, dtype=np.uint64)
    _check(_lib.ssa_debug_aggregates_plan(cp, counts.size, int(msm_slice), int(small_max),
                                          out.ctypes.data_as(C.POINTER(C.c_uint64)), need), "ssa_debug_aggregates_plan")
    w = [int(v) for v in out]
    keys = ("first_aggregate", "aggregates", "first_lane", "lanes", "segment_lanes", "bucket")
    groups = [dict(zip(keys, w[4 + 6 * g:10 + 6 * g])) for g in range(w[2])]
    pos, passes = 4 + 6 * w[2], []
    for _ in range(w[1]):
        cnt = w[pos]
        passes.append([tuple(w[pos + 1 + 4 * d:pos + 5 + 4 * d]) for d in range(cnt)])
        pos += 1 + 4 * cnt
    return {"lanes": w[0], "groups": groups, "passes": passes, "descriptors": w[3]}


def debug_aggregates_fold_plan(counts):
    """host logic of Engine.aggregates (no device needed): (partials in all, pfirst uint64[k + 1]) -- aggregate j shares
    lanes with pfirst[j + 1] - pfirst[j] workgroups of 256 dense lanes; None when refused"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts.size else None
    need = _lib.ssa_debug_aggregates_fold_plan(cp, counts.size, None, 0)
    if need < 0:
        return None
    out = np.zeros(need, dtype=np.uint64)
    _check(_lib.ssa_debug_aggregates_fold_plan(cp, counts.size, out.ctypes.data_as(C.POINTER(C.c_uint64)), need),
           "ssa_debug_aggregates_fold_plan")
    return int(out[0]), out[1:]


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


# ------------------------------------------------------------------------------------------
# Object mirror of the reference's types (thin; bytes in, bytes out)
# ------------------------------------------------------------------------------------------
class PublicKey:
    """PublicKey(AffinePoint) (src/public.rs:24): 96 bytes affine x || y, canonical LE limbs."""

    def __init__(self, affine96, is_identity=False):
        b = bytes(affine96)
        if len(b) != AFFINE_PUBLIC_KEY_LENGTH:
            raise ValueError("PublicKey needs 96 bytes of affine coordinates")
        self.affine = b
        self.is_identity = bool(is_identity)   # AffinePoint::identity() is a valid key (src/public.rs:95-101)

    def verify_signature(self, signature, message):  # src/signature.rs:170-176
        return signature.verify(message, self)

    @classmethod
    def from_private(cls, sk, engine=None):  # impl From<&PrivateKey> for PublicKey, src/public.rs:26-32: [sk]G on the GPU
        return KeyPair.from_private(sk, engine).public_key

    @classmethod
    def from_bytes(cls, b49, engine=None):
        """PublicKey::from_bytes (src/public.rs:54-56): None when decompression fails.  The identity
        encoding decodes to a key whose affine bytes are zero and `is_identity` is set."""
        b = bytes(b49)
        if len(b) != PUBLIC_KEY_LENGTH:
            raise ValueError("compressed public key needs 49 bytes")
        pks, inf, st = (engine or default_engine()).decompress_many(np.frombuffer(b, np.uint8))
        if st[0] != 0:
            return None
        return cls(pks[0].tobytes(), is_identity=bool(inf[0]))

    def to_bytes(self, engine=None):
        """PublicKey::to_bytes (src/public.rs:49-51): x || flag byte, through ssa_compress_many."""
        out, st = (engine or default_engine()).compress_many(np.frombuffer(self.affine, np.uint8),
                                                             pk_inf=np.array([1 if self.is_identity else 0], np.uint8))
        if st[0] != OK:
            raise MalformedInput("PublicKey holds a non-canonical limb")
        return out[0].tobytes()

    def __eq__(self, o):
        return isinstance(o, PublicKey) and o.affine == self.affine and o.is_identity == self.is_identity

    def derive_public(self, chaincode, i, engine=None):
        """PublicKey::derive_public (src/derivation.rs:305-316) -> (PublicKey, ChainCode); a hardened index (the
        reference unwraps a none CtOption and panics) raises MalformedInput"""
        child = ExtendedPublicKey(self, chaincode).derive_normal_public(i, engine)
        if child is None:
            raise MalformedInput("derive_normal_public is none (hardened index or T = O): the reference panics here")
        return child.key, child.chaincode


class PrivateKey:
    """PrivateKey(Scalar) (src/private.rs:25): 32 bytes LE, canonical, non-zero."""

    def __init__(self, scalar32):
        b = bytes(scalar32)
        v = int.from_bytes(b, "little")
        if len(b) != 32 or v == 0 or v >= Q:
            raise ValueError("invalid private key encoding")   # from_bytes is_none, src/private.rs:74-76
        self.bytes = b

    @classmethod
    def new(cls, rng):  # src/private.rs:49-57
        while True:
            v = int.from_bytes(rng(64), "little") % Q
            if v:
                return cls(v.to_bytes(32, "little"))

    def to_bytes(self):
        return self.bytes

    @classmethod
    def from_bytes(cls, b32):  # src/private.rs:74-76: None (CtOption is_none) for a non-canonical or zero scalar
        b = bytes(b32)
        if len(b) != PRIVATE_KEY_LENGTH:
            raise ValueError("private key needs 32 bytes")
        v = int.from_bytes(b, "little")
        return None if v == 0 or v >= Q else cls(b)

    @classmethod
    def from_seed(cls, seed64):  # src/private.rs:79-82: Scalar::from_bytes_wide, None for 0
        b = bytes(seed64)
        if len(b) != 64:
            raise ValueError("seed needs 64 bytes")
        v = int.from_bytes(b, "little") % Q
        return None if v == 0 else cls(v.to_bytes(32, "little"))

    # PrivateKey::sign / sign_and_bind_pkey (src/signature.rs:62-110): "it is faster to sign with a KeyPair" -- here too:
    # the public key is recomputed on the GPU first (PublicKey::from(self))
    def sign(self, message, rng, engine=None):
        return KeyPair.from_private(self, engine).sign(message, rng, engine)

    def sign_and_bind_pkey(self, message, rng, engine=None):
        return KeyPair.from_private(self, engine).sign_and_bind_pkey(message, rng, engine)

    def derive_private(self, chaincode, i, engine=None):
        """PrivateKey::derive_private (src/derivation.rs:291-302) -> (PrivateKey, ChainCode); raises MalformedInput
        where the reference's unwrap would panic (a child key of 0)"""
        child = ExtendedPrivateKey(self, chaincode).derive_private(i, engine)
        if child is None:
            raise MalformedInput("derive_private is none (child key 0): the reference panics here")
        return child.key, child.chaincode

    def __eq__(self, o):
        return isinstance(o, PrivateKey) and o.bytes == self.bytes

    def __hash__(self):
        return hash(self.bytes)


class Signature:
    """Signature{x: CompressedPoint, e: Scalar} (src/signature.rs:34-40), 81 bytes."""

    def __init__(self, sig81):
        b = bytes(sig81)
        if len(b) != SIGNATURE_LENGTH:
            raise ValueError("Signature needs 81 bytes")
        self.bytes = b

    @classmethod
    def from_bytes(cls, b):  # src/signature.rs:217-227: None when e is not canonical
        if int.from_bytes(bytes(b)[49:81], "little") >= Q:
            return None
        return cls(b)

    def to_bytes(self):
        return self.bytes

    def verify(self, message, pkey, engine=None):
        """Ok -> None; otherwise raises SignatureError (src/signature.rs:181-205)."""
        st = (engine or default_engine()).verify_one(self.bytes, pkey.affine, message, check_torsion=True,
                                                     pk_is_identity=pkey.is_identity)
        if st == OK:
            return None
        if st == INVALID_PUBLIC_KEY:
            raise SignatureError(SignatureError.InvalidPublicKey)
        if st == INVALID_SIGNATURE:
            raise SignatureError(SignatureError.InvalidSignature)
        raise MalformedInput("non-canonical field element or scalar (the reference panics here)")

    def __eq__(self, o):
        return isinstance(o, Signature) and o.bytes == self.bytes


class KeyedSignature:
    """KeyedSignature{public_key, signature} (src/signature.rs:55-60); wire form pk(49) || sig(81)."""

    def __init__(self, public_key, signature):
        self.public_key = public_key
        self.signature = signature

    def to_bytes(self, engine=None):  # src/signature.rs:236-243
        return self.public_key.to_bytes(engine) + self.signature.to_bytes()

    @classmethod
    def from_bytes(cls, b130, engine=None):  # src/signature.rs:246-271: None unless both halves decode
        b = bytes(b130)
        if len(b) != KEYED_SIGNATURE_LENGTH:
            raise ValueError("KeyedSignature needs 130 bytes")
        pk = PublicKey.from_bytes(b[:49], engine)
        sig = Signature.from_bytes(b[49:])
        if pk is None or sig is None:
            return None
        return cls(pk, sig)

    def verify(self, message, engine=None):  # src/signature.rs:232-234
        return self.signature.verify(message, self.public_key, engine)

    def __eq__(self, o):
        return isinstance(o, KeyedSignature) and o.public_key == self.public_key and o.signature == self.signature


def pack_keyed_records(engine, sigs, pks, pk_inf=None):
    """n x 130 KeyedSignature records pk(49) || sig(81) from n signatures (81 bytes each) and n affine keys"""
    sigs, pks = _np_u8(sigs).reshape(-1, 81), _np_u8(pks, 96)
    if sigs.shape[0] != pks.shape[0]:
        raise MalformedInput("We should have the same number of signatures than public keys")
    wire = engine.compress_many(pks, pk_inf=pk_inf)[0] if pks.shape[0] else np.zeros((0, 49), np.uint8)
    return np.ascontiguousarray(np.concatenate([np.asarray(wire, dtype=np.uint8).reshape(-1, 49), sigs], axis=1))


class AggregateSignature:
    """The half-aggregate of n signatures: their R's, 49 bytes each, and e_agg = sum a_i e_i mod q
    -- 49 n + 32 bytes for 81 n.  The order of the lanes is part of it."""

    def __init__(self, agg_bytes):
        b = bytes(agg_bytes)
        if len(b) < 32 or (len(b) - 32) % 49:
            raise ValueError("AggregateSignature needs 49 n + 32 bytes")
        self.bytes = b

    def __len__(self):
        return (len(self.bytes) - 32) // 49

    @classmethod
    def aggregate(cls, signatures, public_keys, messages, check=True, engine=None, sliced=False):
        """Engine.aggregate over (signature, public key, message) objects.  check: every signature is verified first
        (verify_batch semantics) and a slice with a bad one raises the SignatureError / MalformedInput of verify_batch.
        sliced: through Engine.aggregate_sliced (any n, the same bytes); engine may be a MultiEngine."""
        packed = _pack_triples(signatures, public_keys, messages)
        if packed is None:
            return cls(bytes(32))
        sigs, pks, inf, flat, off = packed
        eng = engine or default_engine()
        st, agg, _, _ = (eng.aggregate_sliced if sliced else eng.aggregate)(sigs, pks, flat, offsets=off, pk_inf=inf,
                                                                            check=check)
        if st == MALFORMED:
            raise MalformedInput("undecodable signature in batch (the reference panics here)")
        if st != OK:
            raise SignatureError(SignatureError.InvalidSignature)
        return cls(agg.tobytes())

    @classmethod
    def aggregate_valid(cls, signatures, public_keys, messages, engine=None, cache=None):
        """Engine.aggregate_valid over (signature, public key, message) objects -> (the AggregateSignature of the
        triples that verify under verify_batch semantics, the list of their indices).  A triple that does not verify is
        dropped, not raised.  With a KeyCache a triple is kept iff Signature::verify accepts it --
        the subgroup check of its key included, once per key and cache -- so verify_many(..., cache=cache) accepts the
        result; a cache made with wire=True is handed KeyedSignature records."""
        packed = _pack_triples(signatures, public_keys, messages)
        if packed is None:
            return cls(bytes(32)), []
        sigs, pks, inf, flat, off = packed
        eng = engine or (cache.engine if cache is not None else default_engine())
        if cache is None:
            agg, kept = eng.aggregate_valid(sigs, pks, flat, offsets=off, pk_inf=inf)[:2]
        elif cache.wire:
            agg, kept = eng.aggregate_valid_keyed_cached(cache, pack_keyed_records(eng, sigs, pks, inf), flat, offsets=off)[:2]
        else:
            agg, kept = eng.aggregate_valid_cached(cache, sigs, pks, flat, offsets=off, pk_inf=inf)[:2]
        return cls(agg.tobytes()), [int(i) for i in kept]

    @classmethod
    def aggregate_many(cls, batches, check=True, engine=None):
        """Engine.aggregates over a list of (signatures, public keys, messages) slices of objects, one aggregate per
        slice from ONE call -> (list of AggregateSignature, None where aggregate() would raise;
        results uint32[k]: OK, MALFORMED or, with check, the smallest nonzero status of the slice's signatures)"""
        packed = [_pack_triples(*b) for b in batches]
        eng = engine or default_engine()
        flat = [(np.zeros((0, 81), np.uint8), np.zeros((0, 96), np.uint8), [], None) if p is None else
                (p[0], p[1], [bytes(m) for m in b[2]], p[2]) for p, b in zip(packed, batches)]
        aggs, results, _, _ = eng.aggregates(flat, check=check)
        return aggs, results

    def verify(self, public_keys, messages, engine=None, sliced=False):
        """Ok -> None; otherwise raises SignatureError (the equation fails) or MalformedInput.  sliced: through
        Engine.verify_aggregate_sliced (any n, the same verdict); engine may be a MultiEngine."""
        if len(public_keys) != len(self) or len(messages) != len(self):
            raise MalformedInput("We should have the same number of messages than public keys")
        eng = engine or default_engine()
        verify_aggregate = eng.verify_aggregate_sliced if sliced else eng.verify_aggregate
        if len(self) == 0:
            st = verify_aggregate(np.frombuffer(self.bytes, np.uint8), np.zeros((0, 96), np.uint8), None)
        else:
            pks = np.frombuffer(b"".join(p.affine for p in public_keys), np.uint8)
            inf = np.array([1 if p.is_identity else 0 for p in public_keys], np.uint8)
            flat, off = pack_messages(messages)
            st = verify_aggregate(np.frombuffer(self.bytes, np.uint8), pks, flat, offsets=off, pk_inf=inf)
        if st == OK:
            return None
        if st == MALFORMED:
            raise MalformedInput("undecodable aggregate (non-canonical limb or scalar, R or key off the curve)")
        raise SignatureError(SignatureError.InvalidSignature)

    @staticmethod
    def verify_many(aggregates, public_keys, messages, cache=None, engine=None):
        """Many aggregates in one call (DESIGN.md sections 21 and 23): the PublicKey objects and messages of all their
        lanes, in order -> uint32[k], one status per aggregate, each the value verify() stands for on that aggregate
        alone.  With a KeyCache every key's subgroup check is included (INVALID_PUBLIC_KEY for an aggregate that holds a
        key outside the prime-order subgroup) and runs once per key and cache; a cache made with wire=True is handed the
        keys' 49 compressed bytes."""
        eng = engine or (cache.engine if cache is not None else default_engine())
        n = sum(len(a) for a in aggregates)
        if len(public_keys) != n or len(messages) != n:
            raise MalformedInput("We should have the same number of messages than public keys")
        flat, off = pack_messages(messages)
        pks = np.frombuffer(b"".join(p.affine for p in public_keys), np.uint8).reshape(-1, 96)
        inf = np.array([1 if p.is_identity else 0 for p in public_keys], np.uint8)
        if cache is None:
            return eng.verify_aggregates(aggregates, pks, flat, pk_inf=inf, offsets=off)
        if cache.wire:
            wire, _ = eng.compress_many(pks, pk_inf=inf) if n else (np.zeros((0, 49), np.uint8), None)
            return eng.verify_aggregates_cached(cache, aggregates, np.asarray(wire).reshape(-1, 49), flat, offsets=off)[0]
        return eng.verify_aggregates_cached(cache, aggregates, pks, flat, pk_inf=inf, offsets=off)[0]

    def to_bytes(self):
        return self.bytes

    @classmethod
    def from_bytes(cls, b):  # None when the length is not 49 n + 32 or e_agg is not canonical
        b = bytes(b)
        if len(b) < 32 or (len(b) - 32) % 49 or int.from_bytes(b[-32:], "little") >= Q:
            return None
        return cls(b)

    def __eq__(self, o):
        return isinstance(o, AggregateSignature) and o.bytes == self.bytes


class KeyPair:
    """KeyPair{private_key, public_key} (src/keypair.rs:48-53)."""

    def __init__(self, private_key, public_key):
        self.private_key = private_key
        self.public_key = public_key

    @classmethod
    def new(cls, rng, engine=None):  # src/keypair.rs:57-65
        return cls.from_private(PrivateKey.new(rng), engine)

    def to_bytes(self):  # src/keypair.rs:73-75: the private key only; the public key is rebuilt when decoding
        return self.private_key.to_bytes()

    @classmethod
    def from_bytes(cls, b32, engine=None):  # src/keypair.rs:78-89
        sk = PrivateKey.from_bytes(b32)
        return None if sk is None else cls.from_private(sk, engine)

    @classmethod
    def from_seed(cls, seed64, engine=None):  # src/keypair.rs:92-103
        sk = PrivateKey.from_seed(seed64)
        return None if sk is None else cls.from_private(sk, engine)

    def __eq__(self, o):
        return isinstance(o, KeyPair) and o.private_key == self.private_key and o.public_key == self.public_key

    @classmethod
    def from_private(cls, sk, engine=None):  # PublicKey::from(&PrivateKey), src/public.rs:26-32
        eng = engine or default_engine()
        pks = eng.pubkey_many(np.frombuffer(sk.bytes, np.uint8))     # [sk]G and nothing else (no nonce, no response)
        return cls(sk, PublicKey(pks[0].tobytes()))

    def _nonce(self, rng):  # Scalar::random: 64 random bytes mod q, never 0
        while True:
            v = int.from_bytes(rng(64), "little") % Q
            if v:
                return v.to_bytes(32, "little")

    def sign(self, message, rng, engine=None):  # src/signature.rs:114-129 (constant-time, like the reference)
        eng = engine or default_engine()
        msg = np.frombuffer(bytes(message) + b"\0", np.uint8).copy()
        off = np.array([0, len(message)], dtype=np.uint64)
        sk = np.frombuffer(self.private_key.bytes, np.uint8)
        if rng is DEVICE_RNG:
            _, sigs = eng.keygen_sign_many_rng(sk, msg, offsets=off, constant_time=True)
        else:
            _, sigs = eng.keygen_sign_many(sk, np.frombuffer(self._nonce(rng), np.uint8), msg, offsets=off,
                                           constant_time=True)
        return Signature(sigs[0].tobytes())

    def verify_signature(self, signature, message):  # src/signature.rs:159-165
        return signature.verify(message, self.public_key)

    def sign_and_bind_pkey(self, message, rng, engine=None):  # src/signature.rs:132-156
        """the engine emits the 130-byte record pk(49) || sig(81) itself (SSA_FLAG_SIGN_KEYED)"""
        eng = engine or default_engine()
        msg = np.frombuffer(bytes(message) + b"\0", np.uint8).copy()
        off = np.array([0, len(message)], dtype=np.uint64)
        sk = np.frombuffer(self.private_key.bytes, np.uint8)
        if rng is DEVICE_RNG:
            _, recs = eng.keygen_sign_many_rng(sk, msg, offsets=off, constant_time=True, keyed=True)
        else:
            _, recs = eng.keygen_sign_many(sk, np.frombuffer(self._nonce(rng), np.uint8), msg, offsets=off,
                                           constant_time=True, keyed=True)
        return KeyedSignature(self.public_key, Signature(recs[0, 49:].tobytes()))


def _index_bytes(i):
    """an index as the reference's &[u8; 4] (little-endian) from an int or 4 bytes -> uint32"""
    if isinstance(i, (bytes, bytearray, memoryview)):
        b = bytes(i)
        if len(b) != 4:
            raise ValueError("an index is 4 bytes")
        return int.from_bytes(b, "little")
    v = int(i)
    if not 0 <= v < 1 << 32:
        raise ValueError("an index is a 32-bit unsigned value")
    return v


class ChainCode:
    """ChainCode([u8; 32]) (src/derivation.rs:30-31)"""

    def __init__(self, b32):
        b = bytes(b32)
        if len(b) != CHAIN_CODE_LENGTH:
            raise ValueError("ChainCode needs 32 bytes")
        self.bytes = b

    def __eq__(self, o):
        return isinstance(o, ChainCode) and o.bytes == self.bytes

    def __hash__(self):
        return hash(self.bytes)

    def __repr__(self):
        return "ChainCode(%s)" % self.bytes.hex()


class ExtendedPrivateKey:
    """ExtendedPrivateKey{key, chaincode} (src/derivation.rs:46-52); wire form sk(32) || cc(32).  Derivation runs on the
    GPU (ssa_xprv_master_many / ssa_xprv_derive_many); the codecs stay on the host."""

    def __init__(self, key, chaincode):
        self.key = key
        self.chaincode = chaincode if isinstance(chaincode, ChainCode) else ChainCode(chaincode)

    @classmethod
    def generate_master_key(cls, seed, engine=None):  # src/derivation.rs:66-82: None when the key is 0
        b = bytes(seed)
        if len(b) != PRIVATE_KEY_SEED_LENGTH:
            raise ValueError("seed needs 32 bytes")
        out, st = (engine or default_engine()).xprv_master_many(np.frombuffer(b, np.uint8))
        return None if st[0] != OK else cls.from_bytes(out[0].tobytes())

    def derive_private(self, i, engine=None):  # src/derivation.rs:88-92: None when the child key is 0
        out, st = (engine or default_engine()).xprv_derive_many(np.frombuffer(self.to_bytes(), np.uint8),
                                                                [_index_bytes(i)])
        return None if st[0] != OK else ExtendedPrivateKey.from_bytes(out[0].tobytes())

    def derive_public(self, i, engine=None):  # src/derivation.rs:160-174
        out, st = (engine or default_engine()).xprv_derive_many(np.frombuffer(self.to_bytes(), np.uint8),
                                                                [_index_bytes(i)], derive_public=True)
        return None if st[0] != OK else ExtendedPublicKey.from_bytes(out[0].tobytes(), engine)

    def to_bytes(self):  # src/derivation.rs:177-184
        return self.key.to_bytes() + self.chaincode.bytes

    @classmethod
    def from_bytes(cls, b64):  # src/derivation.rs:187-203: None for a non-canonical or zero key
        b = bytes(b64)
        if len(b) != EXTENDED_PRIVATE_KEY_LENGTH:
            raise ValueError("ExtendedPrivateKey needs 64 bytes")
        sk = PrivateKey.from_bytes(b[:32])
        return None if sk is None else cls(sk, ChainCode(b[32:]))

    def __eq__(self, o):
        return isinstance(o, ExtendedPrivateKey) and o.key == self.key and o.chaincode == self.chaincode

    def __hash__(self):
        return hash((self.key.bytes, self.chaincode.bytes))


class ExtendedPublicKey:
    """ExtendedPublicKey{key, chaincode} (src/derivation.rs:207-213); wire form compressed key(49) || cc(32)."""

    def __init__(self, key, chaincode):
        self.key = key
        self.chaincode = chaincode if isinstance(chaincode, ChainCode) else ChainCode(chaincode)

    @classmethod
    def from_extended_private_key(cls, xprv, engine=None):  # src/derivation.rs:225-230
        return cls(PublicKey.from_private(xprv.key, engine), xprv.chaincode)

    def derive_normal_public(self, i, engine=None):
        """src/derivation.rs:235-260: None for a hardened index or T = O; the child may be the identity"""
        out, pks, inf, st = (engine or default_engine()).xpub_derive_many(
            np.frombuffer(self.to_bytes(engine), np.uint8), [_index_bytes(i)])
        if st[0] == MALFORMED:
            raise MalformedInput("ExtendedPublicKey does not encode")
        if st[0] != OK:
            return None
        return ExtendedPublicKey(PublicKey(pks[0].tobytes(), is_identity=bool(inf[0])), ChainCode(out[0, 49:].tobytes()))

    def to_bytes(self, engine=None):  # src/derivation.rs:263-270
        return self.key.to_bytes(engine) + self.chaincode.bytes

    @classmethod
    def from_bytes(cls, b81, engine=None):  # src/derivation.rs:273-290: None when decompression fails or for the identity
        b = bytes(b81)
        if len(b) != EXTENDED_PUBLIC_KEY_LENGTH:
            raise ValueError("ExtendedPublicKey needs 81 bytes")
        pk = PublicKey.from_bytes(b[:49], engine)
        if pk is None or pk.is_identity:
            return None
        return cls(pk, ChainCode(b[49:]))

    def __eq__(self, o):
        return isinstance(o, ExtendedPublicKey) and o.key == self.key and o.chaincode == self.chaincode


def _pack_triples(signatures, public_keys, messages):
    """(signature, public key, message) objects -> the arrays the engine takes (signatures, keys, identity flags,
    messages, offsets), or None for an empty slice; the length checks of the reference's verify_batch"""
    if len(signatures) != len(public_keys):
        raise MalformedInput("We should have the same number of signatures than public keys")
    if len(messages) != len(public_keys):
        raise MalformedInput("We should have the same number of messages than public keys")
    if not signatures:
        return None
    sigs = np.frombuffer(b"".join(s.bytes for s in signatures), np.uint8)
    pks = np.frombuffer(b"".join(p.affine for p in public_keys), np.uint8)
    inf = np.array([1 if p.is_identity else 0 for p in public_keys], np.uint8)
    flat, off = pack_messages(messages)
    return sigs, pks, inf, flat, off


def _status_results(status):
    """statuses of Signature::verify -> None, the SignatureError the reference returns, or a MalformedInput instance"""
    errors = {OK: lambda: None,
              INVALID_PUBLIC_KEY: lambda: SignatureError(SignatureError.InvalidPublicKey),
              INVALID_SIGNATURE: lambda: SignatureError(SignatureError.InvalidSignature),
              MALFORMED: lambda: MalformedInput("non-canonical field element or scalar (the reference panics here)")}
    return [errors[int(st)]() for st in status]


def verify_many(signatures, public_keys, messages, engine=None):
    """Signature::verify (src/signature.rs:181-205) for every (signature, public key, message) of a slice in one call:
    a list with None where the reference returns Ok(()) and the SignatureError it returns otherwise -- not raised; a
    MalformedInput instance where the reference would panic.  Public keys may repeat: each distinct key's subgroup
    check and table run once (Engine.verify_many_dedup)."""
    packed = _pack_triples(signatures, public_keys, messages)
    if packed is None:
        return []
    sigs, pks, inf, flat, off = packed
    eng = engine or default_engine()
    status, _, _ = eng.verify_many_dedup(sigs, pks, flat, offsets=off, check_torsion=True, pk_inf=inf)
    return _status_results(status)


def verify_many_screened(signatures, public_keys, messages, rng=None, engine=None):
    """Signature::verify (src/signature.rs:181-205) for every (signature, public key, message) of a slice, screened on
    the GPU (Engine.verify_many_screened): the list verify_many returns -- None where the
    reference returns Ok(()), the SignatureError it returns otherwise, a MalformedInput instance where it would panic
    -- at about the price of one MSM for an honest slice.  Coefficients from `rng(64)` per signature reduced mod q, or
    drawn on the device when rng is None.  A rejected signature is reported except with the probability stated in
    DESIGN.md section 15."""
    packed = _pack_triples(signatures, public_keys, messages)
    if packed is None:
        return []
    sigs, pks, inf, flat, off = packed
    eng = engine or default_engine()
    coeffs = None
    if rng is not None:
        coeffs = np.frombuffer(b"".join((int.from_bytes(rng(64), "little") % Q).to_bytes(32, "little")
                                        for _ in signatures), np.uint8)
    status, _, _ = eng.verify_many_screened(sigs, pks, flat, offsets=off, check_torsion=True, pk_inf=inf, coeffs=coeffs)
    return _status_results(status)


def verify_many_cached(signatures, public_keys, messages, cache, rng=None, engine=None):
    """verify_many_screened with the public keys' checks kept in `cache` (Engine.keycache_create, DESIGN.md section
    16): the same list, and a key that was seen in an earlier slice or call is not checked again.  The cache belongs to
    the engine that made it: `engine` defaults to it."""
    packed = _pack_triples(signatures, public_keys, messages)
    if packed is None:
        return []
    sigs, pks, inf, flat, off = packed
    eng = engine or cache.engine
    coeffs = None
    if rng is not None:
        coeffs = np.frombuffer(b"".join((int.from_bytes(rng(64), "little") % Q).to_bytes(32, "little")
                                        for _ in signatures), np.uint8)
    status, _, _ = eng.verify_many_cached(cache, sigs, pks, flat, offsets=off, check_torsion=True, pk_inf=inf,
                                          coeffs=coeffs)
    return _status_results(status)


def verify_keyed_many_cached(keyed_signatures, messages, cache, rng=None, engine=None):
    """KeyedSignature::verify (src/signature.rs:232-234) for every (keyed signature, message) of a slice through a key
    cache in wire mode (Engine.keycache_create(capacity, wire=True)): the list verify_many returns.
    A public key seen in an earlier slice or call is neither decompressed nor checked again."""
    if len(messages) != len(keyed_signatures):
        raise MalformedInput("We should have the same number of messages than keyed signatures")
    if not keyed_signatures:
        return []
    eng = engine or cache.engine
    pks = np.frombuffer(b"".join(k.public_key.affine for k in keyed_signatures), np.uint8)
    inf = np.array([1 if k.public_key.is_identity else 0 for k in keyed_signatures], np.uint8)
    comp, st = eng.compress_many(pks, pk_inf=inf)
    if (st != OK).any():
        raise MalformedInput("PublicKey holds a non-canonical limb")
    keyed = np.concatenate([comp, np.frombuffer(b"".join(k.signature.bytes for k in keyed_signatures),
                                                np.uint8).reshape(-1, 81)], axis=1)
    flat, off = pack_messages(messages)
    coeffs = None
    if rng is not None:
        coeffs = np.frombuffer(b"".join((int.from_bytes(rng(64), "little") % Q).to_bytes(32, "little")
                                        for _ in keyed_signatures), np.uint8)
    status, _, _ = eng.verify_keyed_many_cached(cache, keyed, flat, offsets=off, check_torsion=True, coeffs=coeffs)
    return _status_results(status)


def keycache_keep(capacity, u, m, hist):
    """ssa_debug_keycache_keep: (a*, K) of a compaction from the 64 age counts (no device needed)"""
    h = (C.c_uint64 * 64)(*[int(v) for v in hist])
    out = (C.c_uint64 * 2)()
    _check(_lib.ssa_debug_keycache_keep(int(capacity), int(u), int(m), h, out), "ssa_debug_keycache_keep")
    return int(out[0]), int(out[1])


def keycache_plan(capacity, held, u, m):
    """host logic of the key cache (no device): 0 insert the m misses, 1 clear and insert all u keys, 2 bypass"""
    out = C.c_uint32(0)
    _check(_lib.ssa_debug_keycache_plan(int(capacity), int(held), int(u), int(m), C.byref(out)), "ssa_debug_keycache_plan")
    return int(out.value)


def verify_batch_statuses(signatures, public_keys, messages, rng=None, engine=None):
    """verify_batch semantics per signature (screened on the GPU): a uint8 array of statuses, 0 = OK,
    2 = INVALID_SIGNATURE, 3 = MALFORMED (the reference would panic on this input).  Coefficients from `rng(64)` per
    signature reduced mod q, or drawn on the device when rng is None.  A rejected lane is reported except with the
    probability stated in DESIGN.md section 13."""
    if len(signatures) != len(public_keys):
        raise MalformedInput("We should have the same number of signatures than public keys")
    if len(messages) != len(public_keys):
        raise MalformedInput("We should have the same number of messages than public keys")
    if not signatures:
        return np.zeros(0, dtype=np.uint8)
    eng = engine or default_engine()
    sigs = np.frombuffer(b"".join(s.bytes for s in signatures), np.uint8)
    pks = np.frombuffer(b"".join(p.affine for p in public_keys), np.uint8)
    inf = np.array([1 if p.is_identity else 0 for p in public_keys], np.uint8)
    flat, off = pack_messages(messages)
    coeffs = None
    if rng is not None:
        coeffs = np.frombuffer(b"".join((int.from_bytes(rng(64), "little") % Q).to_bytes(32, "little")
                                        for _ in signatures), np.uint8)
    status, _ = eng.verify_batch_screened(sigs, pks, flat, offsets=off, coeffs=coeffs, pk_inf=inf)
    return status


def verify_batch(signatures, public_keys, messages, rng=None, engine=None, msm=False):
    """verify_batch (src/batch.rs:31-50): Ok -> None, else raises SignatureError.
    msm=False: AND of exact per-signature checks (`rng` unused; DESIGN.md, divergence classes).
    msm=True: the reference's own algorithm on the GPU -- random linear combination (coefficients from
    `rng(32)` per signature, or getrandom when rng is None) and a 2n-point MSM."""
    if len(signatures) != len(public_keys):
        raise MalformedInput("We should have the same number of signatures than public keys")
    if len(messages) != len(public_keys):
        raise MalformedInput("We should have the same number of messages than public keys")
    if not signatures:
        return None
    eng = engine or default_engine()
    sigs = np.frombuffer(b"".join(s.bytes for s in signatures), np.uint8)
    pks = np.frombuffer(b"".join(p.affine for p in public_keys), np.uint8)
    inf = np.array([1 if p.is_identity else 0 for p in public_keys], np.uint8)
    flat, off = pack_messages(messages)
    if msm:
        coeffs = None
        if rng is not None:
            coeffs = np.frombuffer(b"".join((int.from_bytes(rng(64), "little") % Q).to_bytes(32, "little")
                                            for _ in signatures), np.uint8)
        st = eng.verify_batch_msm(sigs, pks, flat, offsets=off, coeffs=coeffs, pk_inf=inf)
    else:
        st = eng.verify_batch_status(sigs, pks, flat, offsets=off, check_torsion=False, pk_inf=inf)
    if st == OK:
        return None
    if st == MALFORMED:
        raise MalformedInput("undecodable signature in batch (the reference panics here)")
    raise SignatureError(SignatureError.InvalidSignature)
