"""HIP/CDNA4 kernels exposed to PyTorch (gfx950 only).

* :func:`gemm_nt`, :func:`matmul`, :func:`linear`, :class:`Linear` -- bf16 MFMA GEMM
  (``native/kernels/gemm_bf16.hip``)
* :func:`vector_add`, :func:`transpose_bf16`, :func:`checksum` -- memory-bound
  helpers (``native/kernels/elementwise.hip``)
* :func:`add_rmsnorm`, :func:`rope_qkv_`, :func:`silu_mul`, :func:`attention_qkv` --
  fused decoder-block ops and flash attention (``native/kernels/transformer.hip``,
  ``native/kernels/attention.hip``)
* :func:`flash_attention_qkv`, :func:`attention_qkv_lse`, :func:`attention_qkv_backward` --
  differentiable flash attention: forward with log-sum-exp and the dQ / dK / dV
  kernels (``native/kernels/attention_train.hip``)
* :func:`rmsnorm_residual`, :func:`swiglu`, :func:`rope_qkv`, :func:`softmax_cross_entropy` --
  the differentiable norm, SwiGLU, RoPE and LM loss, over :func:`rmsnorm_backward`,
  :func:`silu_mul_backward`, :func:`cross_entropy_rows` and
  :func:`cross_entropy_rows_backward` (``native/kernels/train_ops.hip``)
* :func:`adamw_table`, :func:`grad_norm`, :func:`adamw_step_` -- the fused AdamW step
  of every tensor of a model over a device-resident tensor table
  (``native/kernels/optimizer.hip``); the optimizer on them is :class:`kgs.optim.AdamW`
* :func:`grad_accumulate_` -- the micro-batches' bf16 gradients summed into fp32 main
  gradients that the step then reads (``native/kernels/grad_accum.hip``)
* :func:`linear_fp8`, :class:`LinearFp8`, :func:`fp8_amax`, :func:`fp8_quantize`, :func:`ref_linear_fp8` --
  a trainable Linear whose forward, dX and dW GEMMs run in e4m3 (``native/kernels/fp8_train.hip``)
* :func:`embedding`, :class:`Embedding`, :func:`embedding_rows`, :func:`embedding_rows_backward` --
  a trainable token embedding: a row gather and a deterministic dense scatter-sum
  (``native/kernels/embedding.hip``)

Importing this package does not touch the GPU; the native library is loaded on
first use and raises :class:`NativeUnavailable` if it is missing.
"""
from ._lib import KernelError, NativeUnavailable, available  # noqa: F401


def __getattr__(name):  # lazy: keep `import kgs.ops` free of torch for CPU-only tools
    if name in ("gemm_nt", "matmul", "linear", "Linear", "fast_path_ok", "transpose", "EPI", "gemm_fp8_nt",
                "quantize_fp8", "gemm_bf16", "quantize_fp8_dev", "Fp8Linear", "gemm_fp8_rows"):
        from . import gemm

        return getattr(gemm, name)
    if name in ("add_rmsnorm", "rms_norm", "rope_qkv_", "rope_tables", "silu_mul", "attention_qkv",
                "attention_qkv_lse", "attention_qkv_backward", "flash_attention_qkv",
                "rmsnorm_backward", "silu_mul_backward", "cross_entropy_rows", "cross_entropy_rows_backward",
                "rmsnorm_residual", "swiglu", "rope_qkv", "softmax_cross_entropy",
                "add_rmsnorm_fp8", "silu_mul_fp8", "quantize_rows_fp8", "argmax_rows", "sample_rows",
                "sample_rows_reference", "penalize_rows", "token_counts_add", "logprob_rows",
                "penalize_rows_reference", "logprob_rows_reference"):
        from . import transformer

        return getattr(transformer, name)
    if name in ("vector_add", "transpose_bf16", "checksum"):
        from . import elementwise

        return getattr(elementwise, name)
    if name in ("adamw_table", "adamw_step_", "grad_norm", "adamw_chunk", "ref_adamw_step", "ref_grad_norm",
                "ref_clip", "grad_accumulate_", "grad_accum_tables_check", "ref_grad_accumulate"):
        from . import optim

        return getattr(optim, name)
    if name in ("fp8_amax", "fp8_quantize", "linear_fp8", "LinearFp8", "ref_linear_fp8", "RefLinearFp8"):
        from . import fp8_train

        return getattr(fp8_train, name)
    if name in ("embedding", "Embedding", "embedding_rows", "embedding_rows_backward", "ref_embedding_rows",
                "ref_embedding_rows_backward"):
        import importlib

        # the op `embedding` shares its name with its module: the module is callable as the op
        mod = importlib.import_module(".embedding", __name__)
        return mod if name == "embedding" else getattr(mod, name)
    raise AttributeError(name)
