"""The autograd wiring of a differentiable op, stated once for its two paths.

``torch.ops.sph3d.<op>`` goes through the dispatcher (schema, fake kernel, opcheck, compile); the public function of the mirrored
module goes around it through a plain ``torch.autograd.Function``, because the ``torch.library`` path costs about four times the
host time per call and a step issues about 230 op calls.  Both are derived here from ONE ``setup`` and ONE ``backward``.
"""
import functools

import torch

WIRED = []       # (registered forward op, the eager apply the module's public function calls), in import order


def differentiable(op, impl, setup, backward, grad_op=None, grad_impl=None):
    """op / impl: the registered forward op and the function it wraps; grad_op / grad_impl: the same pair for the gradient (a tuple
    of each where the backward needs several, None where it needs none).
    setup(ctx, inputs, output) and backward(grad, ctx, *grad_outputs) see either path's context: save_for_backward, saved_tensors,
    needs_input_grad, mark_non_differentiable and plain attributes.  `grad` is grad_op behind the dispatcher and grad_impl on the
    eager path.  -> the eager Function's apply"""
    op.register_autograd(functools.partial(backward, grad_op), setup_context=setup)

    def forward(ctx, *inputs):
        output = impl(*inputs)
        setup(ctx, inputs, output)
        return output

    fn = type(impl.__name__.replace("_impl", "_fn"), (torch.autograd.Function,),
              {"forward": staticmethod(forward), "backward": staticmethod(functools.partial(backward, grad_impl))})
    apply = fn.apply                 # (one bound method: every look at fn.apply makes another)
    WIRED.append((op, apply))
    return apply


def check_graph_ranks(input, nn_index, nn_count):
    """the rank checks of the pooling and un-pooling ops (tf_pool3d.cpp / tf_unpool3d.cpp)"""
    if input.dim() != 3:
        raise ValueError("rank of input should be 3")
    if nn_index.dim() != 3:
        raise ValueError("rank of nn_index should be 3")
    if nn_count.dim() != 2:
        raise ValueError("rank of nn_count should be 2")
