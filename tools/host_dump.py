#!/usr/bin/env python3
"""Print everything the host side of the network decides without a GPU, one value per line, for the library ENDO_HIP_LIB names.

    ENDO_HIP_LIB=/path/to/libendo_hip.so python tools/host_dump.py > dump.txt

The parameter and BatchNorm offsets and the level channels; for a set of shapes the fp32 handle's tape / workspace sizes, group stride and
offsets, the bf16 and the half handle's sizes and offsets, and the forward and backward plans (default options, made-up aligned addresses,
training 1 and 0).  Two builds whose host code lays the network out alike and plans alike print the same bytes: diff the two outputs.
Reads nothing but the library."""

import ctypes
import os
import sys

SHAPES = ((1, 32, 32, 1), (2, 64, 96, 1), (3, 64, 64, 2), (2, 128, 160, 2), (8, 256, 320, 2), (4, 512, 640, 2), (1, 64, 64, 3), (1, 64, 64, 4))
TAPE_PRE, TAPE_BN_SAVED, TAPE_POOL = 0, 1, 2          # ENDO_TAPE_* of include/endo_hip.h
P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def main():
    path = os.environ.get("ENDO_HIP_LIB")
    if not path:
        sys.exit(__doc__)
    lib = ctypes.CDLL(path)

    def fn(name, restype, *argtypes):
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, list(argtypes)
        return f

    for i in range(210):
        print("param_offset %d %d" % (i, fn("endo_net_param_offset", L, I)(i)))
    for i in range(49):
        for which in (0, 1):
            print("bn_offset %d %d %d" % (i, which, fn("endo_net_bn_offset", L, I, I)(i, which)))
    print("param_floats %d" % fn("endo_net_param_floats", L)())
    print("bn_floats %d" % fn("endo_net_bn_floats", L)())
    for level in range(6):
        print("level_channels %d %d" % (level, fn("endo_net_level_channels", I, I)(level)))

    create = fn("endo_net_create_grouped", I, ctypes.POINTER(P), I, I, I, I)
    tape_offset = fn("endo_net_tape_offset", L, P, I, I)
    plan_query = fn("endo_net_plan_query", I, P, I, I, P, P, P, P, P, P, P, I)
    for n, h, w, groups in SHAPES:
        tag = "fp32 %dx%dx%dx%d" % (n, h, w, groups)
        hnd = P()
        rc = create(ctypes.byref(hnd), n, h, w, groups)
        print("%s create %d" % (tag, rc))
        if rc == 0:
            print("%s tape_floats %d" % (tag, fn("endo_net_tape_floats", L, P)(hnd)))
            print("%s gradws_floats %d" % (tag, fn("endo_net_gradws_floats", L, P)(hnd)))
            print("%s group_stride %d" % (tag, fn("endo_net_group_stride", L, P)(hnd)))
            for level in range(6):
                print("%s act_offset %d %d" % (tag, level, fn("endo_net_act_offset", L, P, I)(hnd, level)))
            print("%s tape_offset pre %d" % (tag, tape_offset(hnd, TAPE_PRE, 0)))
            for i in range(49):
                print("%s tape_offset bn_saved %d %d" % (tag, i, tape_offset(hnd, TAPE_BN_SAVED, i)))
            for i in range(5):
                print("%s tape_offset pool %d %d" % (tag, i, tape_offset(hnd, TAPE_POOL, i)))
            raw = (ctypes.c_int32 * 4096)()
            a = [P((i + 1) << 40) for i in range(6)]
            for training in (1, 0):
                for pas in (0, 1):
                    count = plan_query(hnd, pas, training, a[0], a[1], a[2], a[3], a[4], a[5], raw, 4096)
                    print("%s plan pass %d training %d: %d %s" % (tag, pas, training, count, " ".join(str(v) for v in raw[:max(count, 0)])))
            fn("endo_net_destroy", None, P)(hnd)
        for family in ("endo_net16", "endo_net16h"):
            tag16 = "%s %dx%dx%dx%d" % (family, n, h, w, groups)
            hnd = P()
            rc = fn(family + "_create", I, ctypes.POINTER(P), I, I, I, I)(ctypes.byref(hnd), n, h, w, groups)
            print("%s create %d" % (tag16, rc))
            if rc != 0:
                continue
            print("%s tape_bytes %d" % (tag16, fn(family + "_tape_bytes", L, P)(hnd)))
            print("%s bwd_workspace_bytes %d" % (tag16, fn(family + "_bwd_workspace_bytes", L, P)(hnd)))
            offset = fn(family + "_offset", L, P, I, I)
            for what, count in ((0, 1), (1, 49), (2, 5), (3, 6), (4, 6), (5, 6), (6, 6), (7, 1)):
                for i in range(count):
                    print("%s offset %d %d %d" % (tag16, what, i, offset(hnd, what, i)))
            fn(family + "_destroy", None, P)(hnd)


if __name__ == "__main__":
    main()
