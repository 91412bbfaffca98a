"""Which family a kernel name of a rocprofv3 trace belongs to: the BatchNorm and Squeeze-Excite predicates shared by trace_timeline.py and trace_csv_stats.py.

The element-wise passes of csrc/reduce.cpp are instantiations of ONE kernel template, so their trace names differ only in the functor
(`ew_kernel<4, BnApplyF>`, `colreduce_kernel<4, 2, BnBwdF<GradRemask>>`, `tile16_kernel<SeScaleBnF>`).  The predicates keep every launch
in the family the single-purpose kernels it replaced were counted in (DESIGN.md section 3 lists old name -> new name); in particular the
BatchNorm + ReLU + SE-scale pass (once `se_scale_bn_kernel`) stays with the BatchNorm family and the 16-bit tile producers of BnApplyF /
SeScaleBnF stay outside both, as `tile16_kernel<BnApply16F>` / `<SeScaleBn16F>` were."""


def _ew(name, *functors):
    return "ew_kernel" in name and any(f in name for f in functors)


def is_batchnorm(name):
    return "bn_" in name or "BnStat" in name or "BnBwd" in name or "BnRelu" in name or _ew(name, "BnApplyF", "SeScaleBnF")


def is_se(name):      # ask after is_batchnorm
    return "se_" in name or "SeGate" in name or _ew(name, "SeScaleF", "SeBwdApplyF")
