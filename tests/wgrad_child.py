"""Child process of tests/test_wgrad_bf16_gpu.py (not a test module): gsn_wgrad_hip on every case of tests/wgrad_cases.py but the two that are about
the default slab rule, each once with its gathered blocks assembled into plain rows ("/plain") and, where it has gathered blocks, once as it is
("/gathered"); every gW buffer, sentinel bands included, goes into one .npz.  The library reads GSN_WGRAD_PIPE, GSN_WGRAD_WGS and GSN_WGRAD_FP32
once per process, so the parent runs this file once per variant, with GSN_CHAIN_TRACE set, and reads the kernel of every call from stderr: a
line `wgrad case NAME/RUN` goes in front of each call's trace line.

usage: python wgrad_child.py OUT.npz"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import wgrad_cases as wc                                                   # noqa: E402

DEV = torch.device("cuda", 0)


def main(path):
    out = {}
    for name in wc.names(default_process=False):
        case = wc.to_device(wc.build(name), DEV)
        runs = [("plain", wc.assembled(case))]
        if any(i is not None for i in case.idx):
            runs.append(("gathered", case))
        for tag, c in runs:
            buf, gw = wc.gw_buffer(c, DEV)
            sys.stderr.write("wgrad case %s/%s\n" % (name, tag))
            sys.stderr.flush()
            wc.launch(c, gw)
            out["%s/%s" % (name, tag)] = buf.cpu().numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
