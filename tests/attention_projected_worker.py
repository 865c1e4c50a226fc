"""Cases and the C-level call of the projected attention door, shared by tests/test_attention_projected_gpu.py and the child process it starts.

    python tests/attention_projected_worker.py

runs nm_linear_qkv_bf16x3 on AB_CASES in this process and prints one JSON line: the value of NM_GEMM_SMALL it ran under and, per case, the return
code and sha256 digests of the slot buffer's bytes and of q_out's bits.  The switch of csrc/gemm_bf16.hip is read once per process, so the test sets
it in the environment of a fresh child."""
import hashlib
import json
import os
import sys
from pathlib import Path
from typing import NamedTuple

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import kv_slot_util as su  # noqa: E402  (this file's directory: first on the path of a script, put there by pytest for a test module)


class Case(NamedTuple):
    B: int
    S: int
    heads: int
    K: int
    mode: str        # "self": n_q = 32 heads, L = S;  "cross": n_q = 0, queries from the plain GEMM
    L: int
    n_q: int = -1    # -1: what the mode says
    B_att: int = 0   # batch elements the attention checks look at (0: all)

    @property
    def M(self):
        return self.B * self.S

    @property
    def nq(self):
        return self.n_q if self.n_q >= 0 else (32 * self.heads if self.mode == "self" else 0)

    @property
    def id(self):
        return f"{self.mode}-B{self.B}-S{self.S}-L{self.L}-H{self.heads}-K{self.K}" + (f"-nq{self.n_q}" if self.n_q >= 0 else "")


# the small-grid cases of the A/B child: K = 128 and K = 256, self and cross
AB_CASES = [Case(3, 96, 8, 128, "self", 96), Case(5, 96, 4, 256, "self", 96), Case(3, 32, 8, 128, "cross", 65), Case(1, 96, 12, 256, "cross", 129)]


def forms(M, K, n_q, heads, cus):
    """The kernel forms nm_linear_qkv_bf16x3 launches, from its grid arithmetic: row tiles of 128 padded to a multiple of 8, times the 128-column
    chunks of the launch; the small-grid form takes K in {128, 256} and at most 2 x CU count workgroups."""
    cq, ch = n_q // 128, 32 * heads // 128
    grid = lambda chunks: -(-(-(-M // 128)) // 8) * 8 * chunks
    small = lambda chunks: K in (128, 256) and grid(chunks) <= 2 * cus
    if small(cq + 2 * ch):
        return ("small<3>",)
    return ("small<1>" if small(cq + ch) else "ring<1>", "small<2>" if small(ch) else "ring<2>")


def inputs(c):
    return su.inputs(c.M, c.K, c.nq, c.heads)


def project(dev, x, w, c, K=None, n_q=None, heads=None, S=None, M=None):
    """nm_linear_qkv_bf16x3 through _lib on buffers of this call's own: the weight blob packed here, the slot buffer one slot longer than
    nm_attention_workspace_bytes and prefilled with 0xA5, q_out (absent for n_q = 0) four rows longer than M and prefilled with NaN.  The
    keyword arguments replace what the case says (the refusal tests) -- the buffers keep the case's sizes.  -> return code, slots, q_out, on
    the device."""
    from nerfmatch_amd import _lib
    from nerfmatch_amd._lib import dptr

    L = _lib.lib()
    K, n_q, heads, S, M = (c.K if K is None else K, c.nq if n_q is None else n_q, c.heads if heads is None else heads, c.S if S is None else S,
                           c.M if M is None else M)
    xg, wg = x.to(dev).contiguous(), w.to(dev).contiguous()
    N, Kw = wg.shape
    blob = torch.empty(L.nm_linear_blob_bytes_bf16x3(N, Kw), dtype=torch.uint8, device=dev)
    _lib.check(L.nm_linear_pack_bf16x3(dptr(wg), N, Kw, dptr(blob, torch.uint8), _lib.stream()), "nm_linear_pack_bf16x3")
    need = L.nm_attention_workspace_bytes(c.B, c.S, c.heads)
    assert need == c.B * c.heads * (c.S // 32) * su.SLOT_BYTES
    slots = torch.full((need + su.SLOT_BYTES,), 0xA5, dtype=torch.uint8, device=dev)
    q_out = torch.full((c.M + 4, c.nq), float("nan"), device=dev) if c.nq else None
    rc = L.nm_linear_qkv_bf16x3(dptr(xg), dptr(blob, torch.uint8), M, K, n_q, heads, S, dptr(q_out), dptr(slots, torch.uint8), _lib.stream())
    torch.cuda.synchronize()
    return rc, slots, q_out


def digests(slots, q_out):
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    return {"slots": sha(slots), "q": sha(q_out.view(torch.int32)) if q_out is not None else None}


def main():
    dev = torch.device("cuda:0")
    rep = {"NM_GEMM_SMALL": os.environ.get("NM_GEMM_SMALL"), "cases": {}}
    with torch.no_grad():
        for c in AB_CASES:
            t = inputs(c)
            rc, slots, q_out = project(dev, t["x"], t["w"], c)
            rep["cases"][c.id] = dict(digests(slots, q_out), rc=rc)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
