"""The C ABI of libic_amd.so as ctypes prototypes: one line per function that include/ic_amd.h declares, in header order.

This table is the only place in the Python tree where a prototype is written down; tests/test_abi_exports.py parses the
header and compares every entry with its declaration.  Torch-free, so tools and tests can bind a library handle of their own
with bind().
"""
import ctypes

i, u, z, p, s = ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p

# (name, restype, argtypes)
PROTOTYPES = (
    ("icamd_compute_compressed_data_size", z, [i, i, u, u]),
    ("icamd_supports_format", i, [i, i]),
    ("icamd_encoded_size", z, [i, u, u]),
    ("icamd_compress", i, [i, i, i, u, u, u, p, p, z]),
    ("icamd_host_register", i, [p, z]),
    ("icamd_host_unregister", i, [p]),
    ("icamd_compress_and_pad", i, [i, i, i, u, u, u, u, u, p, p, z]),
    ("icamd_pvrtc2_encode_region_device", i, [u, u, u, p, p, p]),
    ("icamd_pvrtc2_workspace_size", z, [u, u]),
    ("icamd_pvrtc4_workspace_size", z, [u, u]),
    ("icamd_pvrtc2_set_workspace", i, [p, z]),
    ("icamd_pvrtc2_tune", i, [i, i]),
    ("icamd_compress_device", i, [i, i, i, u, u, u, p, p, z, p]),
    ("icamd_compress_and_pad_device", i, [i, i, i, u, u, u, u, u, p, p, z, p]),
    ("icamd_encode_device", i, [i, i, i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_encode_etc2_device", i, [i, i, i, i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_etc2_kernel_name", s, [i, i, i]),
    ("icamd_encode_etc2_colour_device", i, [i, i, i, i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_etc2_colour_kernel_name", s, [i, i, i]),
    ("icamd_encode_bc7_device", i, [i, i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_bc7_kernel_name", s, [i, i]),
    ("icamd_decode_device", i, [i, i, u, u, u, u, z, z, p, p, p]),
    ("icamd_decompress", i, [i, i, u, u, u, p, z, p, z]),
    ("icamd_pvrtc2_decompress", i, [u, p, z, p, z]),
    ("icamd_pad_device", i, [i, i, i, u, u, p, u, u, p, z, p]),
    ("icamd_pad_batch_device", i, [i, i, i, u, u, u, p, z, u, u, p, z, z, p]),
    ("icamd_pad", i, [i, i, i, u, u, p, u, u, p, z]),
    ("icamd_downsample_device", i, [i, i, i, u, u, p, p, z, p]),
    ("icamd_downsample_batch_device", i, [i, i, i, u, u, u, p, z, p, z, z, p]),
    ("icamd_downsample", i, [i, i, i, u, u, p, p, z]),
    ("icamd_create_solid_device", i, [i, i, u, u, p, p, z, p]),
    ("icamd_create_solid_batch_device", i, [i, i, u, u, u, p, p, z, z, p]),
    ("icamd_create_solid", i, [i, i, u, u, p, p, z]),
    ("icamd_copy_subimage_device", i, [i, i, u, u, p, u, u, u, u, p, z, p]),
    ("icamd_copy_subimage_batch_device", i, [i, i, u, u, u, p, z, u, u, u, u, p, z, z, p]),
    ("icamd_copy_subimage", i, [i, i, u, u, p, u, u, u, u, p, z]),
    ("icamd_transcode_dxt1_to_etc1_device", i, [p, z, p]),
    ("icamd_transcode_dxt1_to_etc1", i, [p, z]),
    ("icamd_transcode_dxt5_to_etc2_rgba8_device", i, [p, z, p]),
    ("icamd_transcode_dxt5_to_etc2_rgba8", i, [p, z]),
    ("icamd_transcode_dxt1_to_etc2_rgb8_device", i, [p, z, p]),
    ("icamd_transcode_dxt1_to_etc2_rgb8", i, [p, z]),
    ("icamd_transcode_bc4_to_eac_r11_device", i, [p, z, p]),
    ("icamd_transcode_bc4_to_eac_r11", i, [p, z]),
    ("icamd_transcode_bc5_to_eac_rg11_device", i, [p, z, p]),
    ("icamd_transcode_bc5_to_eac_rg11", i, [p, z]),
    ("icamd_compress_batch", i, [i, i, i, u, u, u, u, p, p, z, p, i, p]),
    ("icamd_encode_batch_sharded_device", i, [i, i, i, i, u, u, u, u, p, p, p, i, i, p, z, p]),
    ("icamd_rccl_available", i, []),
    ("icamd_rccl_get_unique_id", i, [p]),
    ("icamd_rccl_comm_init", i, [ctypes.POINTER(p), i, i, p]),
    ("icamd_rccl_comm_destroy", i, [p]),
    ("icamd_gather_blocks_rccl", i, [p, i, i, i, p, p, p, p, p]),
    ("icamd_container_size", z, [i, i, u, u, u]),
    ("icamd_container_write", i, [i, i, u, u, u, p, p, p, z]),
    ("icamd_mip_max_levels", u, [u, u]),
    ("icamd_mip_chain_size", z, [i, u, u, u, p]),
    ("icamd_mip_workspace_size", z, [i, i, u, u, u, u]),
    ("icamd_encode_mips_device", i, [i, i, i, i, u, u, u, u, u, z, z, p, p, p, z, p]),
    ("icamd_mip_pyramid_device", i, [i, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_compress_mips", i, [i, i, i, u, u, u, u, p, p, z]),
    ("icamd_encode_mips_filtered_device", i, [i, i, i, i, i, u, u, u, u, u, z, z, p, p, p, z, p]),
    ("icamd_mip_pyramid_filtered_device", i, [i, i, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_compress_mips_filtered", i, [i, i, i, i, u, u, u, u, p, p, z]),
    ("icamd_mip_kernel_name", s, [i, i, i]),
    ("icamd_etc2_mip_chain_size", z, [i, u, u, u, p]),
    ("icamd_etc2_mip_workspace_size", z, [i, i, u, u, u, u]),
    ("icamd_encode_etc2_mips_device", i, [i, i, i, i, i, i, u, u, u, u, u, z, z, p, p, p, z, p]),
    ("icamd_etc2_mip_kernel_name", s, [i, i, i, i]),
    ("icamd_etc2_mip_tune", i, [i]),
    ("icamd_measure_error_device", i, [i, i, i, u, u, u, u, u, u, z, z, p, p, p, p]),
    ("icamd_measure_error", i, [i, i, u, u, u, p, p, z, p]),
    ("icamd_metric_kernel_name", s, [i, i]),
    ("icamd_encode_eac11_16_device", i, [i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_decode_eac11_16_device", i, [i, u, u, u, u, z, z, p, p, p]),
    ("icamd_measure_error_eac11_16_device", i, [i, i, u, u, u, u, u, u, z, z, p, p, p, p]),
    ("icamd_eac11_16_kernel_name", s, [i, i]),
    ("icamd_eac11_16_metric_kernel_name", s, [i, i]),
    ("icamd_encode_bc6h_device", i, [i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_decode_bc6h_device", i, [i, u, u, u, u, z, z, p, p, p]),
    ("icamd_measure_error_bc6h_device", i, [i, i, u, u, u, u, u, u, z, z, p, p, p, p]),
    ("icamd_bc6h_kernel_name", s, [i, i]),
    ("icamd_bc6h_metric_kernel_name", s, [i, i]),
    ("icamd_encode_bc6h_modes_device", i, [i, i, i, u, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_bc6h_modes_kernel_name", s, [i, i, i]),
    ("icamd_mip_pyramid_f16_device", i, [i, u, u, u, u, u, z, z, p, p, p]),
    ("icamd_mip_f16_kernel_name", s, [i]),
    ("icamd_bptc_mip_chain_size", z, [i, u, u, u, p]),
    ("icamd_bptc_mip_workspace_size", z, [i, i, u, u, u, u]),
    ("icamd_encode_bc7_mips_device", i, [i, i, i, i, u, u, u, u, u, z, z, p, p, p, z, p]),
    ("icamd_encode_bc6h_mips_device", i, [i, i, i, u, u, u, u, u, z, z, p, p, p, z, p]),
    ("icamd_bptc_mip_kernel_name", s, [i, i, i]),
    ("icamd_device_count", i, []),
    ("icamd_last_error", s, []),
    ("icamd_version", s, []),
    ("icamd_kernel_name", s, [i, i]),
    ("icamd_clock_probe_device", i, [p, u, p]),
    ("icamd_wall_clock_rate_khz", u, []),
)
EXPORTS = [name for name, _, _ in PROTOTYPES]


def bind(cdll, allow_missing=False):
    """Sets restype / argtypes of every table entry on the ctypes library handle `cdll` and returns it.  allow_missing: a
    symbol the library lacks is skipped (its later use fails with ctypes' AttributeError) instead of failing here."""
    for name, restype, argtypes in PROTOTYPES:
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            if allow_missing:
                continue
            raise
        fn.restype, fn.argtypes = restype, list(argtypes)
    return cdll
