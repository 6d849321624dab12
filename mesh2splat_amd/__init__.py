def __getattr__(name):
    # mesh2splat_amd.write_ply_compact without importing the converter (numpy, ctypes) with the package
    if name in ("write_ply_compact", "write_ply"):
        from . import converter
        return getattr(converter, name)
    if name == "read_ply_sh":
        from . import gltf_io
        return gltf_io.read_ply_sh
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
