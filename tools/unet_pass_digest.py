#!/usr/bin/env python3
"""One U-Net configuration as bits: the tensor table (name, offset, count) and SHA-256 digests of the prediction, the gradient bucket and the time-embedding
gradient of one forward + backward pass on fixed inputs (parameters uniform at sqrt(3 / fan_in) from fixed seeds, a fixed 10 % dropout mask).  Two builds of
csrc/bla_unet_model.hip compute the same network exactly when every line agrees -- the acceptance check of a host-side change there.
usage: unet_pass_digest.py [--size 16|32] [--batch 1] [--products f32|bf16] [--attention f32|bf16|online] [--heads 1] [--passes 1]
  --size 16: tests/test_unet_model.py's configuration (16 x 16 x 3, widths 32 / 64 / 64 / 48, time 24, key 8: one up-convolution absent, residual 1 x 1s);
  --size 32: the reference's constants (32 x 32 x 3, widths 128 / 256 / 256 / 256, time 512, key 16: bf16 attention and the tiled convolutions apply).
--attention online is BLA_UNET_ATTENTION_BF16_ONLINE; --heads N creates the model with bla_unet_create_heads (N heads of width key in every attention block: the
projections N times as wide) and is printed in the header line when it is not 1.  Together they reach every route of an attention block (csrc/bla_unet_model.hip's
att_route).  Only public entries are called, so the tool also runs against an older build of csrc/.
BLA_UNET_SIDE, BLA_UNET_PADS and BLA_UNET_PREP are read by the library once per process: one run per setting, each a fresh process."""
import argparse, ctypes as C, hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, choices=[16, 32], default=16)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--products", choices=["f32", "bf16"], default="f32")
ap.add_argument("--attention", choices=["f32", "bf16", "online"], default="f32")
ap.add_argument("--heads", type=int, default=1)
ap.add_argument("--passes", type=int, default=1, help="forward + backward passes before the digests (a kernel trace of one pass: 1)")
a = ap.parse_args()
cfg = (dict(image_h=16, image_w=16, in_channels=3, dims=[32, 64, 64, 48], time_dim=24, kernel=3, group_size=32, key_dim=8) if a.size == 16 else
       dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16))
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
B = a.batch
h = bla.unet_create_heads(T.Cfg(cfg["image_h"], cfg["image_w"], cfg["in_channels"], (C.c_int * 4)(*cfg["dims"]), cfg["time_dim"], cfg["kernel"], cfg["group_size"],
                                cfg["key_dim"]), B, bla.UNET_PRODUCTS_BF16 if a.products == "bf16" else bla.UNET_PRODUCTS_F32, a.heads)
if a.attention != "f32":
    bla.unet_set_attention(h, bla.UNET_ATTENTION_BF16 if a.attention == "bf16" else bla.UNET_ATTENTION_BF16_ONLINE)
tensors = []
for i in range(L.bla_unet_tensor_count(h)):
    off, cnt = C.c_size_t(), C.c_size_t(); name = C.create_string_buffer(96)
    chk(L.bla_unet_tensor_info(h, i, C.byref(off), C.byref(cnt), name, 96))
    tensors.append((name.value.decode(), off.value, cnt.value))
shapes = T.shapes_for(tensors, dict(cfg, key_dim=cfg["key_dim"] * a.heads))   # (an attention block's projections: the heads side by side)
total = L.bla_unet_param_count(h); ndrop = L.bla_unet_dropout_count(h)
flat = np.zeros(total, np.float32)
for i, (name, off, cnt) in enumerate(tensors):
    shp = shapes[name]; fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else shp[0]
    scale = 0.05 if name.endswith("biases") else float(np.sqrt(3.0 / fan_in))
    flat[off:off + cnt] = uniform(7000 + i, (cnt,), -scale, scale, np.float32)
chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
image = (B, cfg["in_channels"], cfg["image_h"], cfg["image_w"])
x = bla.to_device(uniform(7921, image, -1, 1, np.float32)); temb = bla.to_device(uniform(7922, (B, cfg["time_dim"]), -1, 1, np.float32))
noise = bla.to_device(uniform(7923, image, -1, 1, np.float32))
drop = bla.DeviceArray((ndrop,), np.uint8).copy_from((uniform(7924, (ndrop,), 0, 1, np.float32) < 0.1).astype(np.uint8))
dtemb = bla.empty((B, cfg["time_dim"]))
for _ in range(a.passes):
    chk(L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, drop.ptr)); chk(L.bla_unet_backward_f32(h, None, noise.ptr))
chk(L.bla_unet_embedding_grad_f32(h, None, dtemb.ptr)); bla.sync()
out = np.empty(image, np.float32); chk(L.bla_memcpy_d2h(out.ctypes.data, L.bla_unet_output(h), out.nbytes, None))
grads = np.empty(total, np.float32); chk(L.bla_memcpy_d2h(grads.ctypes.data, L.bla_unet_grads(h), grads.nbytes, None)); bla.sync()
env = " ".join(f"{k}={os.environ[k]}" for k in ("BLA_UNET_SIDE", "BLA_UNET_PREP", "BLA_UNET_PADS", "BLA_UNET_BF16_PREP") if k in os.environ)
print(f"== {a.size}x{a.size} batch {B} products {a.products} attention {a.attention}{f' heads {a.heads}' if a.heads != 1 else ''} {env}".rstrip())
print(f"parameters {total} dropout decisions {ndrop} tensors {len(tensors)}")
for name, off, cnt in tensors:
    print(f"  {name} {off} {cnt}")
for what, v in (("output", out), ("gradient bucket", grads), ("embedding gradient", dtemb.numpy())):
    assert np.isfinite(v).all() and np.abs(v).max() > 0, what
    print(f"sha256 {what}: {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()}")
chk(L.bla_unet_destroy(h))
