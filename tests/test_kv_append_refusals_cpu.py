"""What the cache writers' C entries refuse before any launch (rsa_kv8_append, rsa_kv8_append_packed, rsa_kv4_append;
csrc/rsa_kv_append.h holds the shared door): one bad argument at a time beside valid ones, and the status each entry gives
for it.  The pointers are made-up
aligned addresses: every case returns before they are read, so this needs no GPU."""
import pytest

from rectified_spaattn_amd import _lib

BAD_ARG, UNSUPPORTED = -1, -2
BASE = 0x10000          # 16-byte aligned and never dereferenced


def _call(entry, **change):
    """The entry over B = 2, Hkv = 2, T = 3, Sk = 128, D = 64, bf16, blocks of 64, contiguous caches, host limits -- with the
    named arguments replaced.  src / dst: (pointer, stride_b, stride_h, stride_s); table: (pointer, stride, num_pages)."""
    a = dict(B=2, Hkv=2, T=3, Sk=128, D=64, dtype=_lib.RSA_BF16, block=64, src=(BASE, 384, 192, 64), dst=(BASE, 16384, 8192, 64),
             table=(None, 0, 0), start_dev=None, start=0, n_new_dev=None, n_new=3)
    a.update(change)
    src, dst = _lib.RsaTensor4(*a["src"]), _lib.RsaOut4(*a["dst"])
    head = (a["B"], a["Hkv"], a["T"], a["Sk"], a["D"], a["dtype"], a["block"], src, src)
    tail = (*a["table"], a["start_dev"], a["start"], a["n_new_dev"], a["n_new"])
    L = _lib.lib()
    if entry == "rsa_kv8_append":
        return L.rsa_kv8_append(*head, dst, dst, *tail, BASE, BASE, None)
    if entry == "rsa_kv8_append_packed":    # (cu_seqlens and the item scratch where n_new stood; k_new's rows through stride_h, stride_s)
        return L.rsa_kv8_append_packed(*head, dst, dst, *tail[:-2], a.get("cu", BASE), BASE, BASE, BASE, None)
    scales = _lib.RsaOut4(BASE, 512, 256, 2)
    return L.rsa_kv4_append(*head, dst, scales, dst, scales, *tail, None)


CASES = [("B = 0", dict(B=0), BAD_ARG),
         ("block = 32", dict(block=32), UNSUPPORTED),
         ("D = 96", dict(D=96), UNSUPPORTED),
         ("dtype neither bf16 nor fp16", dict(dtype=7), UNSUPPORTED),
         ("host start = Sk + 1", dict(start=129), BAD_ARG),
         ("host n_new = T + 1", dict(n_new=4), BAD_ARG),
         ("a negative source stride", dict(src=(BASE, 384, -192, 64)), BAD_ARG),
         ("a destination pointer off by 4 bytes", dict(dst=(BASE + 4, 16384, 8192, 64)), BAD_ARG),
         ("a destination stride of 12", dict(dst=(BASE, 16384, 8192, 12)), BAD_ARG),
         ("a table with num_pages = 0", dict(table=(BASE, 2, 0)), BAD_ARG),
         ("a table with Sk % block != 0", dict(table=(BASE, 2, 4), Sk=100), BAD_ARG),
         ("a device pointer off by 2 bytes", dict(start_dev=BASE + 2), BAD_ARG)]


@pytest.mark.parametrize("entry", ["rsa_kv8_append", "rsa_kv4_append"])
@pytest.mark.parametrize("what,change,status", CASES, ids=[c[0] for c in CASES])
def test_one_bad_argument_gives_its_status_before_any_launch(entry, what, change, status):
    assert _call(entry, **change) == status, (entry, what)


@pytest.mark.parametrize("entry,status", [("rsa_kv8_append", UNSUPPORTED), ("rsa_kv4_append", BAD_ARG)])
def test_the_destination_alignment_is_the_entry_s_own(entry, status):
    """A destination 8 bytes off a 16-byte boundary with a stride of 24: an e4m3 lane's 8-byte store takes it, an MXFP4 lane's
    16-byte store does not.  The extents ask for more than 2^31 - 1 workgroups, the door's last refusal, so the e4m3 entry says
    so (it passed the alignment) and nothing is launched."""
    assert _call(entry, B=2 ** 30, Hkv=2 ** 10, dst=(BASE + 8, 16384, 8192, 24)) == status


@pytest.mark.parametrize("what,change,status", [("no cu_seqlens", dict(cu=None), BAD_ARG), ("block = 32", dict(block=32), UNSUPPORTED),
                                                ("D = 96", dict(D=96), UNSUPPORTED), ("host start = Sk + 1", dict(start=129), BAD_ARG),
                                                ("a destination pointer off by 4 bytes", dict(dst=(BASE + 4, 16384, 8192, 64)), BAD_ARG),
                                                ("a table with num_pages = 0", dict(table=(BASE, 2, 0)), BAD_ARG),
                                                ("cu_seqlens off by 2 bytes in front of block = 32", dict(cu=BASE + 2, block=32), BAD_ARG)],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_the_packed_entry_goes_through_the_same_door_behind_its_own_refusal(what, change, status):
    assert _call("rsa_kv8_append_packed", **change) == status, what


@pytest.mark.parametrize("entry", ["rsa_kv8_append", "rsa_kv4_append"])
def test_two_faults_report_the_first_refusal(entry):
    """The extents are refused in front of the block size, and the block size in front of everything that is a bad argument."""
    assert _call(entry, B=0, block=32) == BAD_ARG
    assert _call(entry, block=32, start=129, dst=(BASE + 4, 16384, 8192, 12)) == UNSUPPORTED
