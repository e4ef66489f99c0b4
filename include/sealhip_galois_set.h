/* sealhip_galois_set.h - Galois sets: many rotations of a batch in one key switch.  An extension of the C ABI of libsealhip.so with a
 * header of its own; include/sealhip.h includes it, so a binding that includes that header has these entry points too.  Conventions
 * (SHL_FUNC, HRESULTs, handles, SealHip_LastError) are those of sealhip.h. */
#ifndef SEALHIP_GALOIS_SET_H
#define SEALHIP_GALOIS_SET_H
#include "sealhip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Galois sets (library extension): many rotations of a batch in one key switch.  The layout "a vector in the slots of one
 * ciphertext" does its linear algebra with rotations - the diagonal method and its baby-step / giant-step form, slot sums,
 * convolutions along the slots - and the inner loop is always "rotate one ciphertext by R different steps".  As R calls of
 * Evaluator_ApplyGalois / RotateVector that is R latency-bound key switches at batch 1; in arithmetic and bytes it is one key switch at
 * batch R in which two things differ per item: the switching key and the automorphism.  The reference has no counterpart (its rotate_*
 * are per object), so the contract is that of every batch extension: each item of the result equals, word for word, the per-object
 * call.  That rules out hoisting (decompose once, permute the raised digits): the reference negates coefficients modulo q_i BEFORE it
 * reduces them modulo q_j, a hoisted form gives other words.  This is the exact form: the same per-item arithmetic, run as one batch.
 * GaloisSet_Create: galois_elts is a host array of count elements.  Validated once, here, with SHL_E_INVALIDARG: count >= 1 and below
 *   2^32; every element odd and below 2 N ("Galois element is not valid"); every element's key present in galois_keys ("Galois key not
 *   present"); galois_keys of this context; a NULL array.  Repeats are allowed.  A NULL context, galois_keys or galois_set is
 *   SHL_E_POINTER.  The set records each key's device slab and uploads one table row (slab, element) per entry with a plain
 *   synchronous copy after draining the device: this is not a hot-path call.
 * GaloisSet_CreateFromSteps: the elements are GaloisTool_GetEltFromStep(steps[r]); a step out of range is refused as there.  A step
 *   of 0 gives an IDENTITY ENTRY - the reference's rotate_internal returns the operand unchanged for 0: such an item is a copy and never
 *   enters the key switch.  A step whose exact key is absent is refused with "Galois key not present": there is NO NAF chain in the set
 *   form - rotate by such a step with Evaluator_RotateVector / RotateRows, which fall back to the chain of power-of-two keys.
 * The keys object must outlive the set.  A call checks on the host that every recorded slab is still the key's current one
 *   (KSwitchKeys_SetKey* and the loads replace it) and fails with SHL_E_INVALIDARG otherwise: make a new set after replacing a key.
 * GaloisSet_Destroy follows ItemMap_Destroy's pool rule: the set may be destroyed right after the call that used it, but not before
 *   the last launch of a graph that recorded it.  GaloisSet_Info: any of the outputs may be NULL; register_order = every key is in the
 *   fused key switch's layout (N >= 2^13), i.e. calls take the one-batch route.
 * Evaluator_ApplyGaloisSet: encrypted is a batch of B items of size 2 in the scheme's native form (CKKS and BGV: NTT form, BFV:
 *   coefficient form), at any level; destination is ANOTHER handle made with Ciphertext_CreateBatch(B * count).  Item b * count + r of
 *   the result equals, word for word, Evaluator_ApplyGalois(item b, galois_elts[r]) on a batch of one - for a set made from steps,
 *   Evaluator_RotateVector / RotateRows by steps[r].  The rotations of one source are adjacent, so Evaluator_DotPlainDevice(..., group =
 *   count) on the result is the diagonal product sum_r pt_r (.) rot_r(ct_b) with no further data movement.  Refused with
 *   SHL_E_INVALIDARG, the destination untouched: destination == encrypted; a destination whose batch is not B * count (B * count must
 *   stay below 2^32); a set or keys of another context; a replaced key; encrypted not of size 2 or not in its native form.  Metadata
 *   (scale, correction factor, is_ntt_form, parms_id), the settle-before-read of an operand with a deferred tail or product pending and
 *   Evaluator_SetTransparentCheck over the result batch are those of Evaluator_ApplyGalois.  All three schemes.  The call makes no
 *   host transfer; it is enqueued on the evaluator's stream and records under Evaluator_BeginCapture.
 *   Route.  A set of one entry is Evaluator_ApplyGalois on the batch, as it stands (measured: the per-item form has nothing to share
 *   there).  More entries, every key in register order (N >= 2^13) and complete: ONE key switch over the B * (entries that are not the identity)
 *   virtual items.  The route rule is asked with that batch, so digit groups (small B * count) and chunks on lanes (large) see the real
 *   amount of work, and a chunk may hold items of several keys.  On the un-split folded sub-route (CKKS, K >= 2) neither pi(c0) nor
 *   pi(c1) is stored: the opening inverse transform and pass 2 read the SOURCE item through the entry's index map, as
 *   Evaluator_ApplyGalois does for one element.  On the other sub-routes the permuted operands go to scratch by virtual item with the
 *   permutation kernel and only the key is per item.  Where that route defers the tail (CKKS / BFV, K >= 2) and the set has no identity
 *   entry, the destination is left with the tail pending exactly as Evaluator_ApplyGalois leaves it: a following Evaluator_RescaleToNext
 *   / ModSwitchToNext on the destination folds as it does today.  With identity entries the key switch runs on the virtual batch in
 *   pool scratch, is completed, and its items are copied into place beside the copies of the operand (device copies on the same
 *   stream).  Smaller rings, keys in natural order, a digit-parallel slice of a key: a host loop over the entries through the
 *   single-key path, each entry's B items copied into place - the call works at every size, only the launch count differs.
 *   Pool scratch on the one-batch route: the key switch's intermediate for B * count items or lanes x chunk of them (Chunked key
 *   switching, below), its sums, and on the permuting sub-routes one plane of B * count items.
 *   Not built: sharing the opening inverse transform across the entries (INTT(pi c1) is a signed permutation of INTT(c1)), NAF chains
 *   inside a set, the digit-parallel multi-GPU forms. */
SHL_FUNC GaloisSet_Create(void *context, void *galois_keys, uint64_t count, const uint32_t *galois_elts, void **galois_set);
SHL_FUNC GaloisSet_CreateFromSteps(void *context, void *galois_keys, uint64_t count, const int *steps, void **galois_set);
SHL_FUNC GaloisSet_Destroy(void *thisptr);
SHL_FUNC GaloisSet_Info(void *thisptr, uint64_t *count, uint64_t *identities, uint64_t *distinct, bool *register_order);
SHL_FUNC Evaluator_ApplyGaloisSet(void *thisptr, void *encrypted, void *galois_set, void *destination);
/* Galois sets (Evaluator_ApplyGaloisSet).  Counters for tests: set calls served by the one-batch route / by the loop over the entries,
 * and fused key-switch launches (one per chunk; an unchunked call issues one whatever the set's count) issued by set calls.  A set
 * call on the one-batch route also counts once in SealHip_GaloisStats, as gathered or permuted by its sub-route. */
SHL_FUNC SealHip_GaloisSetStats(uint64_t *batched, uint64_t *looped, uint64_t *fused_launches);
#ifdef __cplusplus
}
#endif
#endif /* SEALHIP_GALOIS_SET_H */
