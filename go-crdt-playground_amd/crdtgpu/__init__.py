"""crdtgpu -- MI355X batched AWSet / AWSetDelta merge engine (Python host side).

Everything here drives libcrdtgpu.so (HIP kernels for gfx950 behind the C ABI
of include/crdtgpu.h).  Importing fails loudly when the library is missing.
"""

from .abi import (CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY, CRDT_E_DUP_KEY, CRDT_E_HIP, CRDT_E_INVALID, CRDT_E_NOMEM,  # noqa: F401
                  CRDT_E_RCCL, CRDT_E_UNSORTED, CRDT_E_WORKSPACE, CRDT_FOLD_AWSET, CRDT_FOLD_DELTA, CRDT_MAX_OPS_PER_DOC, CRDT_MAX_R, CRDT_MAX_REPLICAS, CRDT_OK,
                  CRDT_OP_ADD, CRDT_OP_DEL, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY,
                  CRDT_DELTA_NONE, CRDT_DELTA_DELTA, CRDT_DELTA_FULL,
                  CRDT_CMP_KEYS, CRDT_CMP_DOTS, CRDT_CMP_A_AHEAD, CRDT_CMP_B_AHEAD, CRDT_DIG_ELEMENTS, CRDT_DIG_STATE,
                  CRDT_DIGEST_GATHER, CRDT_DIGEST_PLACE, CRDT_DIGEST_TREE_FANOUT,
                  CRDT_DIFF_REMOVED, CRDT_DIFF_ADDED, CRDT_DIFF_UPDATED, CRDT_DIFF_CLOCK,
                  CrdtError, LIB_PATH, header_functions, lib, strerror)
from .batch import (AWSetBatch, CompareBuffers, DiffBuffers, DigestTreeBuffers, Headroom, InplaceTarget, MergeLogBuffers, OpBatch, OutBuffers, QueryBatch, QueryBuffers, Replica, ReplicaBuffers, SpillBuffers, SrcBatch, SrcBuffers,  # noqa: F401
                    TombBatch, TombBuffers, repack_slots)
from .engine import (Engine, comm_unique_id, digest_host, digest_tree_host, digest_tree_layout, dump_batch, format_doc, global_context_allreduce,  # noqa: F401
                     load_batch, validate, validate_src)
