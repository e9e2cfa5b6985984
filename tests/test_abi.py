"""CPU-side checks of the C-ABI library: it loads and exports every symbol include/msseg.h declares, and the ctypes table
of hip.py agrees with the header's prototypes."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "msseg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(msseg_[a-z0-9_]+)\s*\(", txt)))


# entry points that ABI version 3 folded into their successors (msseg_ + each name)
_REMOVED_IN_ABI3 = ("dice_ce_partials", "dice_ce_fwd", "dice_ce_finalize", "dice_ce_bwd", "sw_gather_batch_mirror",
                    "sw_blend_batch_mirror", "slab_counts_rule", "pick_voxels_rule", "conv3d_k1_head_dgrad_inbwd",
                    "conv3d_stem_k1_fwd")


def test_library_exports_every_declared_symbol():
    from medicalsemseg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.load_library()
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/msseg.h but not exported"
        assert n in hip.SIGNATURES, f"{n} has no ctypes signature in hip.py"
    assert lib.msseg_abi_version() == 3
    assert not [n for n in _REMOVED_IN_ABI3 if hasattr(lib, "msseg_" + n) or "msseg_" + n in hip.SIGNATURES]
    assert lib.msseg_cout_block(32) == 32 and lib.msseg_cout_block(48) == 48 and lib.msseg_cout_block(3) == 16


def test_signatures_cover_exactly_the_header():
    from medicalsemseg_amd import hip
    assert set(hip.SIGNATURES) == set(_declared())


_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "unsigned": C.c_uint, "msseg_stream_t": C.c_void_p}


def _ctype(ctype, func):
    """ctypes class of a C type as written in include/msseg.h (qualifiers and spacing normalised)"""
    t = " ".join(ctype.replace("const", " ").replace("*", " * ").split())
    if t == "char *":
        return C.c_char_p
    if t == "float *" and func == "msseg_ktimer_get":
        return C.POINTER(C.c_float)
    return C.c_void_p if t.endswith("*") else _SCALARS[t]


def test_signature_types_match_header():
    from medicalsemseg_amd import hip
    txt = open(os.path.join(ROOT, "include", "msseg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    protos = re.findall(r"([\w\s*]+?)\b(msseg_\w+)\s*\(([^()]*)\)\s*;", txt)
    assert {name for _, name, _ in protos} == set(_declared())
    for ret, name, args in protos:
        args = [] if args.strip() == "void" else [re.sub(r"\w+\s*$", "", a) for a in args.split(",")]
        want_args, want_ret = hip.SIGNATURES[name]
        assert len(want_args) == len(args), f"{name}: {len(want_args)} ctypes arguments, {len(args)} in the header"
        for k, (a, w) in enumerate(zip(args, want_args)):
            assert _ctype(a, name) is w, f"{name}: argument {k} is `{a.strip()}` in the header, {w.__name__} in hip.py"
        assert _ctype(ret, name) is want_ret, f"{name}: returns `{ret.strip()}` in the header, {want_ret.__name__} in hip.py"


def test_product_refuses_cpu():
    import torch
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.unet import UNet
    net = UNet(1, 2, (16, 16, 32, 64, 128, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        net((torch.zeros(1, 1, 16, 16, 16), None, None))
    with pytest.raises(RuntimeError, match="GPU only"):
        DiceCELoss()(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_state_dict_layout_matches_monai_names():
    from medicalsemseg_amd.models.unet import UNet
    from oracle.blocks import BasicUNet
    a = UNet(1, 3).state_dict()
    b = BasicUNet(1, 3).state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(a[k].shape == b[k].shape for k in a)
    assert sum(v.numel() for v in a.values()) == 5749443  # BasicUNet 1->3
