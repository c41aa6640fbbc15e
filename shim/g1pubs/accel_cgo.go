// +build cgo,blsmi

// accel_cgo.go: the verify surface of package g1pubs (PublicKey in G1, 96 B; Signature in G2, 192 B) on
// libblsmi.so.
//
// Drop this file into github.com/phoreproject/bls/g1pubs and build with `-tags blsmi`; the upstream
// implementations of Verify, VerifyWithDomain, VerifyAggregate, VerifyAggregateCommon,
// VerifyAggregateCommonWithDomain and VerifyAggregateWithDomain (g1pubs/bls.go:165-174, 252-311) move
// behind `// +build !blsmi`.  bls.go keeps types, Sign, SignWithDomain, PrivToPub, (de)serialisation and
// the aggregation helpers.  tests/test_shim.py checks every C.blsmi_* call below against include/blsmi.h (name, arity and the
// C type of every argument, in order).  Go version: the language of the reference's go.mod (`go 1.13`, /root/reference/go.mod:15)
// -- nothing newer is used (no unsafe.Slice / unsafe.Add, no generics, no `any`, old-style build tags).
package g1pubs

/*
#cgo CFLAGS: -I${SRCDIR}/../../blsmi/include
#cgo LDFLAGS: -L${SRCDIR}/../../blsmi/bls_amd -lblsmi -Wl,-rpath,${SRCDIR}/../../blsmi/bls_amd
#include "blsmi.h"
*/
import "C"

import (
	"errors"
	"strconv"
	"unsafe"

	"github.com/phoreproject/bls"
)

// must: ONE error policy for every entry point.  A non-zero return code is a device / runtime failure (BLSMI_E_HIP, _NOMEM, _RCCL, _ARG:
// include/blsmi.h), never a verdict -- `false` from a Verify* function only ever means that the pairing check failed, as upstream
// (g1pubs/bls.go).  A consensus caller must not mistake a failed hipMalloc for an invalid signature: panic, like upstream does on its own
// internal errors (a deployment that prefers to degrade wraps the call sites in recover() and re-runs them on the upstream CPU path).
func must(rc C.int, what string) {
	if rc != 0 {
		panic("blsmi: " + what + " failed (" + strconv.Itoa(int(rc)) + ")")
	}
}

// Compile-time layout guards: the *_jac entry points read the structs below as 36 / 18 contiguous uint64 (x, y, z; FQ2 = two FQ; FQ =
// FQRepr = [6]uint64: g2.go:298-302, g1.go:252-256, fq2.go:14-17, fq.go:11-13, fqrepr.go:14).  If upstream ever changes a layout the
// index below is no longer the constant 0 and the package stops compiling (constant index out of range / constant overflow) instead of
// handing the device garbage.
var _ = [1]struct{}{}[unsafe.Sizeof(bls.G2Projective{})-288]
var _ = [1]struct{}{}[unsafe.Sizeof(bls.G1Projective{})-144]
var _ = [1]struct{}{}[unsafe.Sizeof(bls.FQRepr{})-48]

func init() {
	must(C.blsmi_init_devices(0), "init_devices (no usable MI355X, or RCCL missing on a multi-GPU node)")
}

func u8(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// The points cross the boundary AS THE GO HEAP HOLDS THEM (blsmi 0.6, the *_jac entry points): a *bls.G1Projective is 18 contiguous
// uint64 -- x, y, z, each FQ 6 little-endian Montgomery limbs (g1.go:252-256, fq.go:11-13, fqrepr.go:14) -- and a *bls.G2Projective 36
// (g2.go:298-302).  One 144 / 288-byte copy per point: no ToAffine (an Fq inversion, g1.go:322-340 -- run even at z = 1), no
// SerializeBytes (MontReduce + byte swap, g1.go:157-167) on a host core; the library runs ToAffine on the device.  z == 0 is the point at
// infinity there (G1Projective.IsZero, g1.go:287-289), so no flag bytes travel either.

// packKeys: n*18 uint64, the public keys' G1Projective structs.
func packKeys(pubs []*PublicKey) []C.uint64_t {
	pk := make([]C.uint64_t, 18*len(pubs))
	for i := range pubs {
		copy(pk[18*i:18*i+18], (*[18]C.uint64_t)(unsafe.Pointer(pubs[i].p))[:])
	}
	return pk
}

// packSigs: n*36 uint64, the signatures' G2Projective structs.
func packSigs(sigs []*Signature) []C.uint64_t {
	sg := make([]C.uint64_t, 36*len(sigs))
	for i := range sigs {
		copy(sg[36*i:36*i+36], (*[36]C.uint64_t)(unsafe.Pointer(sigs[i].s))[:])
	}
	return sg
}

func u64(b []C.uint64_t) *C.uint64_t {
	if len(b) == 0 {
		return nil
	}
	return &b[0]
}

// sigWords: the one signature of an aggregate call, in place (plain memory without Go pointers: cgo may read it directly).
func sigWords(s *Signature) *C.uint64_t {
	return (*C.uint64_t)(unsafe.Pointer(s.s))
}

func packMsgs(msgs [][]byte) (m []byte, off []C.uint64_t) {
	off = make([]C.uint64_t, len(msgs)+1)
	for i, x := range msgs {
		m = append(m, x...)
		off[i+1] = C.uint64_t(len(m))
	}
	if len(m) == 0 {
		m = []byte{0}
	}
	return
}

// VerifyBatch: n independent Verify() in one call (g1pubs/bls.go:165-168 per tuple).
func VerifyBatch(msgs [][]byte, pubs []*PublicKey, sigs []*Signature) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_jac(u8(m), &off[0], u64(pk), u64(sg), u8(ok), nil, C.size_t(n)), "g1pubs_verify_batch_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// ValidatePublicKeys: out[i] = pubs[i] is on the curve and in the prime-order subgroup (IsOnCurve && IsInCorrectSubgroupAssumingOnCurve,
// true for infinity as upstream) -- what the randomised batch verifications and the default multiplications presuppose and Deserialize*
// guarantees.  For keys built any other way; the points go over as they lie, nothing is inverted (INTEGRATION.md 2l).
func ValidatePublicKeys(pubs []*PublicKey) []bool {
	n := len(pubs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	pk := packKeys(pubs)
	st := make([]byte, n)
	must(C.blsmi_g1_check_batch_jac(u64(pk), 1, u8(st), C.size_t(n)), "g1_check_batch_jac")
	for i := range st {
		out[i] = st[i] == C.BLSMI_POINT_OK || st[i] == C.BLSMI_POINT_INFINITY
	}
	return out
}

// ValidateSignatures: the same for signatures.
func ValidateSignatures(sigs []*Signature) []bool {
	n := len(sigs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	sg := packSigs(sigs)
	st := make([]byte, n)
	must(C.blsmi_g2_check_batch_jac(u64(sg), 1, u8(st), C.size_t(n)), "g2_check_batch_jac")
	for i := range st {
		out[i] = st[i] == C.BLSMI_POINT_OK || st[i] == C.BLSMI_POINT_INFINITY
	}
	return out
}

// VerifyBatchRandomized gives VerifyBatch's verdicts from ONE pairing check over the whole batch (small-exponent batch
// verification: the library draws fresh random 64-bit weights per call; INTEGRATION.md 2g).  When the check holds every tuple is
// true; when it fails the library computes the per-tuple verdicts.  Keys and signatures must lie in the prime-order subgroups,
// as Deserialize* leaves them.
func VerifyBatchRandomized(msgs [][]byte, pubs []*PublicKey, sigs []*Signature) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_rlc_jac(u8(m), &off[0], u64(pk), u64(sg), nil, u8(ok), nil, C.size_t(n), nil), "g1pubs_verify_batch_rlc_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyBatchRandomizedLocate is VerifyBatchRandomized for input an adversary may have touched (INTEGRATION.md 2l): when the combined
// check fails, one pairing equation per block of `block` tuples (0: the library chooses; else even and at least 2) finds the blocks that
// hold, and only the tuples of the others go through the per-tuple path.  Verdicts as VerifyBatch; an odd block panics, as every
// library error does.
func VerifyBatchRandomizedLocate(msgs [][]byte, pubs []*PublicKey, sigs []*Signature, block int) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_rlc_locate_jac(u8(m), &off[0], u64(pk), u64(sg), nil, C.size_t(block), u8(ok), nil, C.size_t(n), nil, nil),
		"g1pubs_verify_batch_rlc_locate_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyBatchRandomizedGrouped is VerifyBatchRandomized for tuples that share messages (an attestation subnet, a slot, a sync
// committee): msgs is a table of d messages and tuple i is (msgs[msgIdx[i]], pubs[i], sigs[i]).  The tuples of one message share one
// pairing of the combined check -- d hashes and Miller loops instead of n (INTEGRATION.md 2g) -- and the verdicts are those of
// VerifyBatchRandomized on the expanded messages.  An index outside the table panics, as every library error does.
func VerifyBatchRandomizedGrouped(msgs [][]byte, msgIdx []uint32, pubs []*PublicKey, sigs []*Signature) []bool {
	n := len(msgIdx)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_rlc_grouped_jac(u8(m), &off[0], C.size_t(len(msgs)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])),
		u64(pk), u64(sg), nil, u8(ok), nil, C.size_t(n), nil), "g1pubs_verify_batch_rlc_grouped_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyBatchRandomizedGroupedLocate is VerifyBatchRandomizedGrouped for input an adversary may have touched (INTEGRATION.md 2k): the
// tuples of every message are cut into cells of at most `block` tuples (0: the library chooses; any other value >= 1 is taken), the
// combined check runs over the cells' sums, and when it fails one pairing equation per cell finds the cells that hold -- only the
// tuples of the others go through the per-tuple path.  Verdicts as VerifyBatch on the expanded messages.
func VerifyBatchRandomizedGroupedLocate(msgs [][]byte, msgIdx []uint32, pubs []*PublicKey, sigs []*Signature, block int) []bool {
	n := len(msgIdx)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac(u8(m), &off[0], C.size_t(len(msgs)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])),
		u64(pk), u64(sg), nil, C.size_t(block), u8(ok), nil, C.size_t(n), nil, nil), "g1pubs_verify_batch_rlc_grouped_locate_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// Verify keeps the upstream signature (g1pubs/bls.go:165).
func Verify(m []byte, pub *PublicKey, sig *Signature) bool {
	return VerifyBatch([][]byte{m}, []*PublicKey{pub}, []*Signature{sig})[0]
}

// VerifyWithDomain keeps the upstream signature (g1pubs/bls.go:171).
func VerifyWithDomain(m [32]byte, pub *PublicKey, sig *Signature, domain [8]byte) bool {
	return VerifyWithDomainBatch([][32]byte{m}, []*PublicKey{pub}, []*Signature{sig}, domain)[0]
}

// VerifyWithDomainBatch: out[i] = VerifyWithDomain(msgs[i], pubs[i], sigs[i], domain).
func VerifyWithDomainBatch(msgs [][32]byte, pubs []*PublicKey, sigs []*Signature, domain [8]byte) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_with_domain_batch_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), u64(sg), u8(ok), nil, C.size_t(n)), "g1pubs_verify_with_domain_batch_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyWithDomainBatchRandomized gives VerifyWithDomainBatch's verdicts from one pairing check (VerifyBatchRandomized).
func VerifyWithDomainBatchRandomized(msgs [][32]byte, pubs []*PublicKey, sigs []*Signature, domain [8]byte) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_with_domain_batch_rlc_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), u64(sg), nil, u8(ok), nil, C.size_t(n), nil), "g1pubs_verify_with_domain_batch_rlc_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyWithDomainBatchRandomizedLocate is VerifyWithDomainBatchRandomized that finds the bad tuples by blocks (VerifyBatchRandomizedLocate).
func VerifyWithDomainBatchRandomizedLocate(msgs [][32]byte, pubs []*PublicKey, sigs []*Signature, domain [8]byte, block int) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), u64(sg), nil, C.size_t(block), u8(ok), nil, C.size_t(n), nil, nil), "g1pubs_verify_with_domain_batch_rlc_locate_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyWithDomainBatchRandomizedGrouped is VerifyWithDomainBatchRandomized over a table of d messages and n indices into it
// (VerifyBatchRandomizedGrouped).
func VerifyWithDomainBatchRandomizedGrouped(msgs [][32]byte, msgIdx []uint32, pubs []*PublicKey, sigs []*Signature, domain [8]byte) []bool {
	n := len(msgIdx)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(msgs) == 0 {
		panic("blsmi: VerifyWithDomainBatchRandomizedGrouped: empty message table")
	}
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		C.size_t(len(msgs)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])), u64(pk), u64(sg), nil, u8(ok), nil, C.size_t(n), nil),
		"g1pubs_verify_with_domain_batch_rlc_grouped_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyWithDomainBatchRandomizedGroupedLocate is VerifyWithDomainBatchRandomizedGrouped that finds the bad tuples by cells
// (VerifyBatchRandomizedGroupedLocate).
func VerifyWithDomainBatchRandomizedGroupedLocate(msgs [][32]byte, msgIdx []uint32, pubs []*PublicKey, sigs []*Signature, domain [8]byte, block int) []bool {
	n := len(msgIdx)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(msgs) == 0 {
		panic("blsmi: VerifyWithDomainBatchRandomizedGroupedLocate: empty message table")
	}
	pk := packKeys(pubs)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		C.size_t(len(msgs)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])), u64(pk), u64(sg), nil, C.size_t(block), u8(ok), nil, C.size_t(n), nil, nil),
		"g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyAggregate keeps the upstream signature (g1pubs/bls.go:252): length check here, duplicate
// rejection in the library.
func (s *Signature) VerifyAggregate(pubKeys []*PublicKey, msgs [][]byte) bool {
	if len(pubKeys) != len(msgs) {
		return false
	}
	m, off := packMsgs(msgs)
	pk := packKeys(pubKeys) // a key or the signature at infinity (z == 0): verdict false (upstream panics in MillerLoop)
	var ok C.int
	must(C.blsmi_g1pubs_verify_aggregate_jac(u8(m), &off[0], u64(pk), sigWords(s), C.size_t(len(msgs)), &ok), "g1pubs_verify_aggregate_jac")
	return ok != 0
}

// VerifyAggregateCommon keeps the upstream signature (g1pubs/bls.go:287).
func (s *Signature) VerifyAggregateCommon(pubKeys []*PublicKey, msg []byte) bool {
	if C.blsmi_prefer_cpu(C.BLSMI_SHAPE_POINT_ADD, C.size_t(len(pubKeys))) != 0 {
		return Verify(msg, AggregatePublicKeys(pubKeys), s) // a handful of keys: sum them on the upstream path
	}
	pk := packKeys(pubKeys)
	one := []byte{0}
	mp := u8(msg)
	if len(msg) == 0 {
		mp = u8(one)
	}
	var ok C.int
	must(C.blsmi_g1pubs_verify_aggregate_common_jac(mp, C.size_t(len(msg)), u64(pk), sigWords(s), C.size_t(len(pubKeys)), &ok), "g1pubs_verify_aggregate_common_jac")
	return ok != 0
}

// VerifyAggregateCommonWithDomain keeps the upstream signature (g1pubs/bls.go:294).
func (s *Signature) VerifyAggregateCommonWithDomain(pubKeys []*PublicKey, msg [32]byte, domain [8]byte) bool {
	pk := packKeys(pubKeys)
	var ok C.int
	must(C.blsmi_g1pubs_verify_aggregate_common_with_domain_jac((*C.uint8_t)(unsafe.Pointer(&msg[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), sigWords(s), C.size_t(len(pubKeys)), &ok), "g1pubs_verify_aggregate_common_with_domain_jac")
	return ok != 0
}

// VerifyAggregateWithDomain keeps the upstream signature (g1pubs/bls.go:300); no duplicate check upstream
// either.  (Upstream on zero messages compares Pairing(G1One, sig) with 1 -- true only for the infinity
// signature, where it panics first; the shim returns false.)
func (s *Signature) VerifyAggregateWithDomain(pubKeys []*PublicKey, msgs [][32]byte, domain [8]byte) bool {
	if len(pubKeys) != len(msgs) {
		return false
	}
	if len(msgs) == 0 {
		return false
	}
	pk := packKeys(pubKeys)
	var ok C.int
	must(C.blsmi_g1pubs_verify_aggregate_with_domain_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), sigWords(s), C.size_t(len(msgs)), &ok), "g1pubs_verify_aggregate_with_domain_jac")
	return ok != 0
}

// SumPublicKeys is AggregatePublicKeys (g1pubs/bls.go:192-204) for large sets: the points are summed on the device as they are and the sum
// comes back as a G1Projective (z = 1; the reference's G1ProjectiveZero for the empty or cancelling sum).
func SumPublicKeys(pubKeys []*PublicKey) *PublicKey {
	if C.blsmi_prefer_cpu(C.BLSMI_SHAPE_POINT_ADD, C.size_t(len(pubKeys))) != 0 {
		return AggregatePublicKeys(pubKeys)
	}
	pk := packKeys(pubKeys)
	out := new(bls.G1Projective)
	var inf C.int
	must(C.blsmi_g1_sum_jac(u64(pk), C.size_t(len(pubKeys)), (*C.uint64_t)(unsafe.Pointer(out)), &inf), "g1_sum_jac")
	return &PublicKey{p: out}
}

// SumSignatures is AggregateSignatures (g1pubs/bls.go:177-189) the same way.
func SumSignatures(sigs []*Signature) *Signature {
	if C.blsmi_prefer_cpu(C.BLSMI_SHAPE_POINT_ADD, C.size_t(len(sigs))) != 0 {
		return AggregateSignatures(sigs)
	}
	sg := packSigs(sigs)
	out := new(bls.G2Projective)
	var inf C.int
	must(C.blsmi_g2_sum_jac(u64(sg), C.size_t(len(sigs)), (*C.uint64_t)(unsafe.Pointer(out)), &inf), "g2_sum_jac")
	return &Signature{s: out}
}

// VerifySerializedBatch: DeserializePublicKey + DeserializeSignature + Verify for n tuples in one device
// pass, from the 48 / 96-byte Serialize() forms (g1pubs/bls.go:18-20, 67-69), subgroup checks included.
func VerifySerializedBatch(msgs [][]byte, pubs [][48]byte, sigs [][96]byte) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_serialized_batch(u8(m), &off[0],
		(*C.uint8_t)(unsafe.Pointer(&pubs[0])), (*C.uint8_t)(unsafe.Pointer(&sigs[0])), 1,
		u8(ok), nil, nil, C.size_t(n)), "g1pubs_verify_serialized_batch")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

func secretBytes(keys []*SecretKey) []byte {
	sk := make([]byte, 0, 32*len(keys))
	for i := range keys {
		kb := keys[i].Serialize() // 32 bytes big-endian
		sk = append(sk, kb[:]...)
	}
	return sk
}

// sigsFromWords: the library hands signatures back as G2Projective records (z = 1; the reference's zero point for sk = 0 mod r): one copy each.
func sigsFromWords(sg []C.uint64_t, n int) []*Signature {
	out := make([]*Signature, n)
	for i := range out {
		p := new(bls.G2Projective)
		copy((*[36]C.uint64_t)(unsafe.Pointer(p))[:], sg[36*i:36*i+36])
		out[i] = &Signature{s: p}
	}
	return out
}

// SignBatch is the batch form of Sign (g1pubs/bls.go:132-135): out[i] = keys[i] * HashG2(msgs[i]), one library call.  Small batches stay
// on the upstream CPU path (blsmi_prefer_cpu); the secret scalars cross the PCIe bus otherwise.
func SignBatch(msgs [][]byte, keys []*SecretKey) []*Signature {
	n := len(msgs)
	if n == 0 {
		return nil
	}
	if C.blsmi_prefer_cpu(C.BLSMI_SHAPE_SIGN, C.size_t(n)) != 0 {
		out := make([]*Signature, n)
		for i := range msgs {
			out[i] = Sign(msgs[i], keys[i])
		}
		return out
	}
	m, off := packMsgs(msgs)
	sg := make([]C.uint64_t, 36*n)
	must(C.blsmi_g1pubs_sign_batch_jac(u8(m), &off[0], u8(secretBytes(keys)), &sg[0], C.size_t(n)), "g1pubs_sign_batch_jac")
	return sigsFromWords(sg, n)
}

// SignWithDomainBatch: out[i] = SignWithDomain(msgs[i], keys[i], domain) (g1pubs/bls.go:138-141).
func SignWithDomainBatch(msgs [][32]byte, keys []*SecretKey, domain [8]byte) []*Signature {
	n := len(msgs)
	if n == 0 {
		return nil
	}
	sg := make([]C.uint64_t, 36*n)
	must(C.blsmi_g1pubs_sign_with_domain_batch_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u8(secretBytes(keys)), &sg[0], C.size_t(n)), "g1pubs_sign_with_domain_batch_jac")
	return sigsFromWords(sg, n)
}

// VerifyAggregateCommonBatch is the batch form of VerifyAggregateCommon (blsmi 0.9): out[j] = sigs[j].VerifyAggregateCommon(committees[j],
// msgs[j]) in one library call -- the m committee sums run on the device beside the hash of the m messages, then one verify batch.
func VerifyAggregateCommonBatch(sigs []*Signature, committees [][]*PublicKey, msgs [][]byte) []bool {
	n := len(sigs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(committees) != n || len(msgs) != n {
		panic("blsmi: VerifyAggregateCommonBatch: length mismatch")
	}
	seg := make([]C.uint64_t, n+1) // committee j = keys[seg[j]:seg[j+1]]: the idx = NULL form
	var keys []*PublicKey
	for j, c := range committees {
		keys = append(keys, c...)
		seg[j+1] = seg[j] + C.uint64_t(len(c))
	}
	m, off := packMsgs(msgs)
	pk := packKeys(keys)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_aggregate_common_batch_jac(u8(m), &off[0], u64(pk), C.size_t(len(keys)), nil, &seg[0], u64(sg), u8(ok), nil, C.size_t(n)),
		"g1pubs_verify_aggregate_common_batch_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyAggregateCommonWithDomainBatch: out[j] = sigs[j].VerifyAggregateCommonWithDomain(committees[j], msgs[j], domain) in one call.
func VerifyAggregateCommonWithDomainBatch(sigs []*Signature, committees [][]*PublicKey, msgs [][32]byte, domain [8]byte) []bool {
	n := len(sigs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(committees) != n || len(msgs) != n {
		panic("blsmi: VerifyAggregateCommonWithDomainBatch: length mismatch")
	}
	seg := make([]C.uint64_t, n+1) // committee j = keys[seg[j]:seg[j+1]]: the idx = NULL form
	var keys []*PublicKey
	for j, c := range committees {
		keys = append(keys, c...)
		seg[j+1] = seg[j] + C.uint64_t(len(c))
	}
	pk := packKeys(keys)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac((*C.uint8_t)(unsafe.Pointer(&msgs[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		u64(pk), C.size_t(len(keys)), nil, &seg[0], u64(sg), u8(ok), nil, C.size_t(n)), "g1pubs_verify_aggregate_common_with_domain_batch_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// messageTable puts equal messages into the table once: msgs[j] is table[idx[j]].
func messageTable(msgs [][]byte) (table [][]byte, idx []uint32) {
	at := make(map[string]uint32, len(msgs))
	idx = make([]uint32, len(msgs))
	for j, m := range msgs {
		k, seen := at[string(m)]
		if !seen {
			k = uint32(len(table))
			at[string(m)] = k
			table = append(table, m)
		}
		idx[j] = k
	}
	return table, idx
}

// VerifyAggregateCommonBatchRandomized is VerifyAggregateCommonBatch under ONE pairing equation (blsmi 0.16; INTEGRATION.md 2n): the
// library draws a random 64-bit weight per item, and one Miller loop per distinct message and one final exponentiation stand for the m
// checks.  Equal messages are put into the table once here.  The verdicts are VerifyAggregateCommonBatch's: when the equation fails, or a
// committee is empty or sums to infinity, they come from its m checks.
func VerifyAggregateCommonBatchRandomized(sigs []*Signature, committees [][]*PublicKey, msgs [][]byte) []bool {
	n := len(sigs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(committees) != n || len(msgs) != n {
		panic("blsmi: VerifyAggregateCommonBatchRandomized: length mismatch")
	}
	seg := make([]C.uint64_t, n+1) // committee j = keys[seg[j]:seg[j+1]]: the idx = NULL form
	var keys []*PublicKey
	for j, c := range committees {
		keys = append(keys, c...)
		seg[j+1] = seg[j] + C.uint64_t(len(c))
	}
	table, msgIdx := messageTable(msgs)
	m, off := packMsgs(table)
	pk := packKeys(keys)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac(u8(m), &off[0], C.size_t(len(table)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])),
		u64(pk), C.size_t(len(keys)), nil, &seg[0], u64(sg), nil, u8(ok), nil, C.size_t(n), nil), "g1pubs_verify_aggregate_common_batch_rlc_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// VerifyAggregateCommonWithDomainBatchRandomized is VerifyAggregateCommonWithDomainBatch under one pairing equation
// (VerifyAggregateCommonBatchRandomized).
func VerifyAggregateCommonWithDomainBatchRandomized(sigs []*Signature, committees [][]*PublicKey, msgs [][32]byte, domain [8]byte) []bool {
	n := len(sigs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	if len(committees) != n || len(msgs) != n {
		panic("blsmi: VerifyAggregateCommonWithDomainBatchRandomized: length mismatch")
	}
	seg := make([]C.uint64_t, n+1) // committee j = keys[seg[j]:seg[j+1]]: the idx = NULL form
	var keys []*PublicKey
	for j, c := range committees {
		keys = append(keys, c...)
		seg[j+1] = seg[j] + C.uint64_t(len(c))
	}
	at := make(map[[32]byte]uint32, n)
	var table [][32]byte
	msgIdx := make([]uint32, n)
	for j, m := range msgs {
		k, seen := at[m]
		if !seen {
			k = uint32(len(table))
			at[m] = k
			table = append(table, m)
		}
		msgIdx[j] = k
	}
	pk := packKeys(keys)
	sg := packSigs(sigs)
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac((*C.uint8_t)(unsafe.Pointer(&table[0])), (*C.uint8_t)(unsafe.Pointer(&domain[0])),
		C.size_t(len(table)), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])), u64(pk), C.size_t(len(keys)), nil, &seg[0], u64(sg), nil, u8(ok), nil, C.size_t(n), nil),
		"g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}

// ---- the wire format in batches (blsmi 0.15; INTEGRATION.md 2m) --------------------------------------------------------------------------
// Keys and signatures arrive and leave compressed (48 / 96 bytes, g1pubs/bls.go:18-20, 67-69).  Upstream deserialises one element per call on a
// host core -- a square root plus the r * P subgroup walk -- and serialises through one Fq inversion per point; the functions below do either for
// n elements in one library call, between the compressed bytes and the G?Projective structs as the Go heap holds them.

// decodeErrors: the messages of upstream's Decompress* and subgroup check, by the error code of blsmi_g?_decompress_batch.
var decodeErrors = [5]string{"", "unexpected compression mode", "unexpected information in compressed infinity", "point not on curve", "not in correct subgroup"}

// DeserializePublicKeys is DeserializePublicKey (g1pubs/bls.go) for n keys, subgroup check included: out[i] is nil where errs[i] is not.
func DeserializePublicKeys(b [][48]byte) ([]*PublicKey, []error) {
	n := len(b)
	out := make([]*PublicKey, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	pk := make([]C.uint64_t, 18*n)
	ec := make([]byte, n)
	must(C.blsmi_g1_decompress_batch_jac((*C.uint8_t)(unsafe.Pointer(&b[0])), 1, &pk[0], nil, u8(ec), C.size_t(n)), "g1_decompress_batch_jac")
	for i := range out {
		if ec[i] != 0 {
			errs[i] = errors.New(decodeErrors[ec[i]])
			continue
		}
		p := new(bls.G1Projective)
		copy((*[18]C.uint64_t)(unsafe.Pointer(p))[:], pk[18*i:18*i+18])
		out[i] = &PublicKey{p: p}
	}
	return out, errs
}

// DeserializeSignatures is DeserializeSignature for n signatures, the same way.
func DeserializeSignatures(b [][96]byte) ([]*Signature, []error) {
	n := len(b)
	out := make([]*Signature, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	sg := make([]C.uint64_t, 36*n)
	ec := make([]byte, n)
	must(C.blsmi_g2_decompress_batch_jac((*C.uint8_t)(unsafe.Pointer(&b[0])), 1, &sg[0], nil, u8(ec), C.size_t(n)), "g2_decompress_batch_jac")
	for i := range out {
		if ec[i] != 0 {
			errs[i] = errors.New(decodeErrors[ec[i]])
			continue
		}
		p := new(bls.G2Projective)
		copy((*[36]C.uint64_t)(unsafe.Pointer(p))[:], sg[36*i:36*i+36])
		out[i] = &Signature{s: p}
	}
	return out, errs
}

// SerializePublicKeys is PublicKey.Serialize for n keys: the structs go over as they lie, the inversion and the compression run on the device.
func SerializePublicKeys(pubs []*PublicKey) [][48]byte {
	n := len(pubs)
	out := make([][48]byte, n)
	if n == 0 {
		return out
	}
	pk := packKeys(pubs)
	must(C.blsmi_g1_compress_batch_jac(u64(pk), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(n)), "g1_compress_batch_jac")
	return out
}

// SerializeSignatures is Signature.Serialize for n signatures.
func SerializeSignatures(sigs []*Signature) [][96]byte {
	n := len(sigs)
	out := make([][96]byte, n)
	if n == 0 {
		return out
	}
	sg := packSigs(sigs)
	must(C.blsmi_g2_compress_batch_jac(u64(sg), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(n)), "g2_compress_batch_jac")
	return out
}

// VerifySerializedBatchRandomized gives VerifySerializedBatch's verdicts by VerifyBatchRandomizedLocate: both inputs are deserialised on the
// device, subgroup check included, and go through the combined check as the in-memory points they then are.  An element that does not
// deserialise is the zero point there: its tuple is false and only its own block of `block` tuples (0: the library chooses; else even and at
// least 2) goes through the per-tuple path.
func VerifySerializedBatchRandomized(msgs [][]byte, pubs [][48]byte, sigs [][96]byte, block int) []bool {
	n := len(msgs)
	out := make([]bool, n)
	if n == 0 {
		return out
	}
	m, off := packMsgs(msgs)
	pk := make([]C.uint64_t, 18*n)
	sg := make([]C.uint64_t, 36*n)
	ec := make([]byte, n)
	must(C.blsmi_g1_decompress_batch_jac((*C.uint8_t)(unsafe.Pointer(&pubs[0])), 1, &pk[0], nil, u8(ec), C.size_t(n)), "g1_decompress_batch_jac")
	must(C.blsmi_g2_decompress_batch_jac((*C.uint8_t)(unsafe.Pointer(&sigs[0])), 1, &sg[0], nil, u8(ec), C.size_t(n)), "g2_decompress_batch_jac")
	ok := make([]byte, n)
	must(C.blsmi_g1pubs_verify_batch_rlc_locate_jac(u8(m), &off[0], u64(pk), u64(sg), nil, C.size_t(block), u8(ok), nil, C.size_t(n), nil, nil),
		"g1pubs_verify_batch_rlc_locate_jac")
	for i := range ok {
		out[i] = ok[i] != 0
	}
	return out
}
