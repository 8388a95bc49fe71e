"""What the host-side tests of the C ABI hand an entry point in place of device memory: every call they make returns before
anything is launched, so a descriptor is only inspected and a pointer only tested for NULL and alignment."""
from spatially_aware_ai_amd import _abi

P = 4096  # a non-NULL, 256-byte aligned stand-in for a device pointer


def fake_volume(n=8, dim=0, dtype=_abi.SAF_F32, **fields):
    """A saf_volume of n^3 voxels with every buffer and axis table at P; `fields` overrides members by name (None: NULL)."""
    v = _abi.SafVolume()
    v.nx = v.ny = v.nz = n
    v.feat_dim, v.feat_dtype = dim, dtype
    for f in ("axis_x", "axis_y", "axis_z", "tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
        setattr(v, f, P)
    for f, val in fields.items():
        setattr(v, f, val)
    return v
