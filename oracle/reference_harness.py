"""oracle/reference_harness.py — TEST INFRASTRUCTURE ONLY; usable where build() has byte-compiled the reference
modules into oracle/_ref/ (build_ref(), out of git), or where the reference tree itself exists.

Loads the UNMODIFIED reference modules from /root/reference/ring_flash_attn under the private
package name `ref_ring_flash_attn`:
  * a namespace stub replaces the package's __init__ (whose `adapters` import is broken against
    transformers 5.x: hf_adapter.py:9-19), so only the algorithm modules are imported;
  * `flash_attn.flash_attn_interface` — the CUDA-only dependency that is absent here — is
    provided by the CPU oracle (oracle/flash_attn_ref.py), or (provider="shim") by the repo's own
    `flash_attn` compatibility package.
This is "the reference's CPU path" (BASELINE.md §3): reference schedule + merge + communication
code, executed under gloo, with the restated attention arithmetic underneath.  It is used to
generate the golden fixtures in tests/golden/ (tests/golden/make_golden.py).
Bytecode writing is disabled so nothing is dropped into the read-only reference tree.
"""
import importlib
import os
import py_compile
import sys
import types

REF_ROOT = os.environ.get("RFA_REFERENCE_ROOT", "/root/reference")
REF_BUILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref")     # build_ref()'s output

_MODULES = [
    "utils",
    "ring_flash_attn",
    "zigzag_ring_flash_attn",
    "ring_flash_attn_varlen",
    "zigzag_ring_flash_attn_varlen",
    "llama3_flash_attn_varlen",
    "stripe_flash_attn",
]


def _package_dir():
    """the reference's package directory: the byte-compiled copy build_ref() made, else the reference tree, else None"""
    for d, ext in ((os.path.join(REF_BUILD, "ring_flash_attn"), ".pyc"), (os.path.join(REF_ROOT, "ring_flash_attn"), ".py")):
        if all(os.path.isfile(os.path.join(d, m + ext)) for m in _MODULES):
            return d
    return None


def available():
    return _package_dir() is not None


def build_ref():
    """byte-compile the reference's algorithm modules (unmodified) into oracle/_ref/ring_flash_attn/<module>.pyc, so
    that the tests load them from the repository tree; nothing to do where the reference tree is absent.  Returns the
    output directory or None."""
    src = os.path.join(REF_ROOT, "ring_flash_attn")
    if not os.path.isdir(src):
        return None
    dst = os.path.join(REF_BUILD, "ring_flash_attn")
    os.makedirs(dst, exist_ok=True)
    for m in _MODULES:
        py_compile.compile(os.path.join(src, m + ".py"), cfile=os.path.join(dst, m + ".pyc"), doraise=True,
                           invalidation_mode=py_compile.PycInvalidationMode.UNCHECKED_HASH)
    return dst


def load_reference(provider="oracle"):
    """returns dict name -> reference module.

    provider = "oracle": `flash_attn` is the CPU restatement (oracle/flash_attn_ref.py) — the golden
    generator.  provider = "shim": `flash_attn` is THIS repo's compatibility package
    (ring-flash-attention_amd/shims/flash_attn, INTEGRATION.md route B) — used by the test that runs the
    unmodified reference schedules through the shipped operator interface (fresh process only: the
    reference modules bind `flash_attn` at import time)."""
    if not available():
        raise RuntimeError(f"reference modules not found ({REF_BUILD}: run build(); or the tree at {REF_ROOT})")
    sys.dont_write_bytecode = True
    if provider == "shim":
        pkg_root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ring-flash-attention_amd")
        for p in (pkg_root, os.path.join(pkg_root, "shims")):     # ring_flash_attn (backend) + the opt-in flash_attn shim
            if p not in sys.path:
                sys.path.insert(0, p)
        if getattr(sys.modules.get("flash_attn"), "_rfa_oracle_stub", False) or "ref_ring_flash_attn" in sys.modules:
            raise RuntimeError("load_reference(provider='shim') needs a process that has not loaded the oracle stub")
        import flash_attn  # noqa: F401  (the shipped compatibility package)
        import flash_attn.flash_attn_interface  # noqa: F401
    else:
        _install_oracle_stub()

    if "ref_ring_flash_attn" not in sys.modules:
        pkg = types.ModuleType("ref_ring_flash_attn")
        pkg.__path__ = [_package_dir()]
        sys.modules["ref_ring_flash_attn"] = pkg
    return {m: importlib.import_module("ref_ring_flash_attn." + m) for m in _MODULES}


def _install_oracle_stub():
    from . import flash_attn_ref as R

    if "flash_attn" not in sys.modules or not getattr(sys.modules["flash_attn"], "_rfa_oracle_stub", False):
        fa = types.ModuleType("flash_attn")
        fa._rfa_oracle_stub = True
        fai = types.ModuleType("flash_attn.flash_attn_interface")
        for name in R.__all__:
            setattr(fai, name, getattr(R, name))
        fa.flash_attn_interface = fai
        sys.modules["flash_attn"] = fa
        sys.modules["flash_attn.flash_attn_interface"] = fai
