// Package crdtgpu is the MI355X merge path for package crdt
// (rsms/go-crdt-playground), bound over cgo to libcrdtgpu.so (include/crdtgpu.h).
//
// UNTESTED HERE: the build image has no Go toolchain, so this file is neither
// compiled nor run in this repository. It is the source a maintainer adds next
// to the reference package. Every rule in it is exercised through the same C ABI
// by the Python mirror (go-crdt-playground_amd/crdtgpu/awset.py,
// tests/test_scenarios_gpu.py, tests/test_mirror_width.py) and the C++ mirror
// (go-crdt-playground_amd/host/crdt.hpp, tests/cpp/test_scenarios.cpp).
//
// It keeps the reference types and adds batch entry points:
//
//	(*AWSet).Merge       awset.go:103-161           -> Engine.Merge / MergeBatch
//	both directions      awset.go:103 twice          -> Engine.ExchangeBatch (one snapshot)
//	ordered AWSet merges awset.go:103, in order      -> Engine.FoldBatch
//	(*AWSetDelta).Merge  awset-delta_test.go:51-166  -> Engine.DeltaMerge / DeltaMergeBatch
//	MakeDeltaMergeData   awset-delta_test.go:79-105  -> Engine.DeltaBatch (what to send a peer)
//	resident replicas    (no reference counterpart)  -> Engine.SourcesBatch (fold / extraction input on the device)
//	                                                    Engine.ReplicaSelect / ReplicaScatter (documents moved with Deleted and actors)
//	                                                    Engine.ReplicaScatterInPlace (merged documents written back where they fit)
//
// AWSetDelta lives in a _test.go file of the reference, invisible to importers,
// so this package defines it (with Del and Clone, awset-delta_test.go:9-49).
//
// Needs Go >= 1.21 (min/max builtins, unsafe.SliceData).
//
// Host arrays come from crdt_host_alloc (page-locked C memory): the C structs
// handed to the library then hold C pointers only, as cgo's pointer rules
// require, and the uploads run at full PCIe rate.
package crdtgpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../go-crdt-playground_amd/crdtgpu -lcrdtgpu -Wl,-rpath,${SRCDIR}/../../go-crdt-playground_amd/crdtgpu
#include "crdtgpu.h"
*/
import "C"

import (
	"fmt"
	"sort"
	"unsafe"

	crdt "github.com/rsms/go-crdt-playground" // the reference package (no go.mod upstream: adjust the path)
)

// ---------------------------------------------------------------- engine

// Engine is one library context (one per goroutine that issues calls).
type Engine struct{ ctx *C.crdt_ctx }

// NewEngine opens a context on a HIP device.
func NewEngine(device int) (*Engine, error) {
	var ctx *C.crdt_ctx
	if rc := C.crdt_ctx_create(C.int(device), &ctx); rc != 0 {
		return nil, errOf("crdt_ctx_create", rc)
	}
	return &Engine{ctx}, nil
}

// Close releases the context and its device workspaces.
func (e *Engine) Close() {
	if e.ctx != nil {
		C.crdt_ctx_destroy(e.ctx)
		e.ctx = nil
	}
}

// Error is a library error; Code is a CRDT_E_* value. CRDT_E_ACTOR_RANGE is
// where the reference panics (HasDot / Counter at actor == len(vv),
// crdt-misc.go:29,37).
type Error struct {
	Call string
	Code int
}

func (e *Error) Error() string {
	return fmt.Sprintf("%s: %s", e.Call, C.GoString(C.crdt_strerror(C.int(e.Code))))
}

func errOf(call string, rc C.int) error { return &Error{call, int(rc)} }

// ---------------------------------------------------------------- AWSetDelta

// AWSetDelta is the reference's delta-state set (awset-delta_test.go:9-12).
type AWSetDelta struct {
	crdt.AWSet
	Deleted map[string]crdt.Dot
}

// Del removes keys with one fresh dot for the whole call, recorded as a
// tombstone for each key that was present (awset-delta_test.go:14-33).
func (s *AWSetDelta) Del(keys ...string) {
	s.VersionVector[s.Actor]++
	dot := crdt.Dot{Actor: s.Actor, Counter: s.VersionVector[s.Actor]}
	for _, k := range keys {
		if _, ok := s.Entries[k]; !ok {
			continue
		}
		if s.Deleted == nil {
			s.Deleted = map[string]crdt.Dot{}
		}
		s.Deleted[k] = dot
		delete(s.Entries, k)
	}
}

// Clone is a deep copy (awset-delta_test.go:35-49).
func (s *AWSetDelta) Clone() *AWSetDelta {
	c := &AWSetDelta{AWSet: crdt.AWSet{Actor: s.Actor}}
	c.VersionVector = append(crdt.VersionVector(nil), s.VersionVector...)
	c.Entries = make(map[string]crdt.Dot, len(s.Entries))
	for k, d := range s.Entries {
		c.Entries[k] = d
	}
	if len(s.Deleted) > 0 {
		c.Deleted = make(map[string]crdt.Dot, len(s.Deleted))
		for k, d := range s.Deleted {
			c.Deleted[k] = d
		}
	}
	return c
}

// ---------------------------------------------------------------- page-locked arrays

type arena struct {
	blocks []unsafe.Pointer
	err    error
}

func (a *arena) alloc(bytes int) unsafe.Pointer {
	if bytes < 8 {
		bytes = 8
	}
	var p unsafe.Pointer
	if a.err == nil {
		if rc := C.crdt_host_alloc(C.size_t(bytes), &p); rc != 0 {
			a.err = errOf("crdt_host_alloc", rc)
			return nil
		}
		a.blocks = append(a.blocks, p)
	}
	return p
}

func (a *arena) u64(n int) []uint64 {
	p := a.alloc(n * 8)
	if p == nil {
		return make([]uint64, n) // never handed to C: a.err is set
	}
	return unsafe.Slice((*uint64)(p), n)
}

func (a *arena) u32(n int) []uint32 {
	p := a.alloc(n * 4)
	if p == nil {
		return make([]uint32, n)
	}
	return unsafe.Slice((*uint32)(p), n)
}

func (a *arena) free() {
	for _, p := range a.blocks {
		C.crdt_host_free(p)
	}
	a.blocks = nil
}

func p64(s []uint64) *C.uint64_t { return (*C.uint64_t)(unsafe.Pointer(unsafe.SliceData(s))) }
func p32(s []uint32) *C.uint32_t { return (*C.uint32_t)(unsafe.Pointer(unsafe.SliceData(s))) }

// ---------------------------------------------------------------- interning

// docKeys interns one document's keys: a key's id is its rank in string order
// among every key of the document's states. The kernels compare keys of one
// document only, so this is the exact order-preserving bijection they need,
// built from one small sort per document (no batch-wide map).
type docKeys []string

func internDoc(maps ...map[string]crdt.Dot) docKeys {
	seen := map[string]struct{}{}
	var ks docKeys
	for _, m := range maps {
		for k := range m {
			if _, ok := seen[k]; !ok {
				seen[k] = struct{}{}
				ks = append(ks, k)
			}
		}
	}
	sort.Strings(ks)
	return ks
}

func (ks docKeys) id(k string) uint64 { return uint64(sort.SearchStrings(ks, k)) }

// entries is a run of (key id, actor, counter) arrays in C memory.
type entries struct {
	keys     []uint64
	actors   []uint32
	counters []uint64
}

func (a *arena) entries(n int) entries { return entries{a.u64(n), a.u32(n), a.u64(n)} }

// put writes m's entries, ascending by id, at e[at:]; returns the next position.
func (e entries) put(at int, m map[string]crdt.Dot, ks docKeys) int {
	ids := make([]uint64, 0, len(m))
	for k := range m {
		ids = append(ids, ks.id(k))
	}
	sort.Slice(ids, func(i, j int) bool { return ids[i] < ids[j] })
	for _, id := range ids {
		d := m[ks[id]]
		e.keys[at], e.actors[at], e.counters[at] = id, uint32(d.Actor), uint64(d.Counter)
		at++
	}
	return at
}

func putVV(dst []uint64, vv crdt.VersionVector) {
	for i := range dst {
		dst[i] = 0
		if i < len(vv) {
			dst[i] = uint64(vv[i])
		}
	}
}

// out is one merge output: document d's live entries are
// [offsets[d], offsets[d] + counts[d]), its clock vv[d*R : d*R+R].
type out struct {
	offsets, counts []uint32
	e               entries
	vv              []uint64
	c               C.crdt_awset_out
}

func (a *arena) out(n, R, slots int) *out {
	o := &out{offsets: a.u32(n + 1), counts: a.u32(n), e: a.entries(slots + 1), vv: a.u64(n * R)}
	o.c = C.crdt_awset_out{offsets: p32(o.offsets), counts: p32(o.counts), keys: p64(o.e.keys),
		actors: p32(o.e.actors), counters: p64(o.e.counters), vv: p64(o.vv)}
	return o
}

// apply writes document d of the output into dst (entries replaced, clock of
// width w: VersionVector.Merge appends the longer tail, crdt-misc.go:43-55).
func (o *out) apply(d, R, w int, ks docKeys, dst *crdt.AWSet) {
	m := make(map[string]crdt.Dot, o.counts[d])
	for j := o.offsets[d]; j < o.offsets[d]+o.counts[d]; j++ {
		m[ks[o.e.keys[j]]] = crdt.Dot{Actor: crdt.Actor(o.e.actors[j]), Counter: uint(o.e.counters[j])}
	}
	dst.Entries = m
	vv := make(crdt.VersionVector, w)
	for r := 0; r < w; r++ {
		vv[r] = uint(o.vv[d*R+r])
	}
	dst.VersionVector = vv
}

// batch packs one AWSet state per document.
func (a *arena) batch(states []*crdt.AWSet, keys []docKeys, R int) (C.crdt_awset_batch, []uint32) {
	n, total := len(states), 0
	for _, s := range states {
		total += len(s.Entries)
	}
	off, e, vv := a.u32(n+1), a.entries(total), a.u64(n*R)
	at := 0
	for d, s := range states {
		off[d] = uint32(at)
		if a.err == nil {
			at = e.put(at, s.Entries, keys[d])
			putVV(vv[d*R:(d+1)*R], s.VersionVector)
		}
	}
	off[n] = uint32(total)
	return C.crdt_awset_batch{n_docs: C.uint32_t(n), R: C.uint32_t(R), offsets: p32(off),
		keys: p64(e.keys), actors: p32(e.actors), counters: p64(e.counters), vv: p64(vv)}, off
}

// ---------------------------------------------------------------- joins

// Merge is dst.Merge(src) (awset.go:103) on the GPU: a one-document batch
// (two PCIe round trips; batch many documents per call for throughput).
func (e *Engine) Merge(dst, src *crdt.AWSet) error {
	return e.MergeBatch([]*crdt.AWSet{dst}, []*crdt.AWSet{src})
}

// MergeBatch does dsts[i].Merge(srcs[i]) for every i in one call
// (same logic as host/crdt.hpp MergeBatch, tested on the GPU by tests/cpp/test_scenarios.cpp)
// (crdt_awset_join_batch). Destinations must be distinct. Every merge reads
// the states as they were when the call began (a source that is also a
// destination of the batch is read before it changes).
func (e *Engine) MergeBatch(dsts, srcs []*crdt.AWSet) error {
	if len(dsts) != len(srcs) {
		return fmt.Errorf("MergeBatch: %d destinations, %d sources", len(dsts), len(srcs))
	}
	n := len(dsts)
	if n == 0 {
		return nil
	}
	if err := distinct(dsts); err != nil {
		return err
	}
	docs := make([][]docState, n)
	keys := make([]docKeys, n)
	widths := make([]int, n)
	for i := range dsts {
		docs[i] = []docState{stateOf(dsts[i], nil), stateOf(srcs[i], nil)}
		keys[i] = internDoc(dsts[i].Entries, srcs[i].Entries)
		widths[i] = max(len(dsts[i].VersionVector), len(srcs[i].VersionVector))
	}
	R, err := raggedChecks(false, docs)
	if err != nil {
		return err
	}
	var a arena
	defer a.free()
	cd, doff := a.batch(dsts, keys, R)
	cs, soff := a.batch(srcs, keys, R)
	o := a.out(n, R, int(doff[n])+int(soff[n]))
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_awset_join_batch(e.ctx, &cd, &cs, &o.c); rc != 0 {
		return errOf("crdt_awset_join_batch", rc)
	}
	for i, dst := range dsts {
		o.apply(i, R, widths[i], keys[i], dst)
	}
	return nil
}

// ExchangeBatch is anti-entropy both ways in one call
// (same logic as host/crdt.hpp ExchangeBatch, tested on the GPU by tests/cpp/test_scenarios.cpp
// and timed by tests/cpp/boundary_bench.cpp)
// (crdt_awset_exchange_batch): for every i, as[i] becomes
// as[i].Clone().Merge(bs[i]) and bs[i] becomes bs[i].Clone().Merge(as[i]), the
// two merges of ONE snapshot, from one read of the pair. This is not the
// reference's sequential round trip a.Merge(b); b.Merge(a) (awset_test.go:15-16),
// in which the second merge sees the updated a.
func (e *Engine) ExchangeBatch(as, bs []*crdt.AWSet) error {
	if len(as) != len(bs) {
		return fmt.Errorf("ExchangeBatch: %d and %d states", len(as), len(bs))
	}
	n := len(as)
	if n == 0 {
		return nil
	}
	if err := distinct(append(append([]*crdt.AWSet(nil), as...), bs...)); err != nil {
		return err
	}
	docs := make([][]docState, 0, 2*n)
	keys := make([]docKeys, n)
	widths := make([]int, n)
	for i := range as {
		docs = append(docs, []docState{stateOf(as[i], nil), stateOf(bs[i], nil)},
			[]docState{stateOf(bs[i], nil), stateOf(as[i], nil)})
		keys[i] = internDoc(as[i].Entries, bs[i].Entries)
		widths[i] = max(len(as[i].VersionVector), len(bs[i].VersionVector))
	}
	R, err := raggedChecks(false, docs)
	if err != nil {
		return err
	}
	var a arena
	defer a.free()
	ca, aoff := a.batch(as, keys, R)
	cb, boff := a.batch(bs, keys, R)
	slots := int(aoff[n]) + int(boff[n])
	oab, oba := a.out(n, R, slots), a.out(n, R, slots)
	if a.err != nil {
		return a.err
	}
	// both directions hold the same keys at the same slots: one key column,
	// written and downloaded once (include/crdtgpu.h, crdt_awset_exchange_*)
	oba.e.keys = oab.e.keys
	oba.c.keys = oab.c.keys
	if rc := C.crdt_awset_exchange_batch(e.ctx, &ca, &cb, &oab.c, &oba.c); rc != 0 {
		return errOf("crdt_awset_exchange_batch", rc)
	}
	for i := range as {
		oab.apply(i, R, widths[i], keys[i], as[i])
		oba.apply(i, R, widths[i], keys[i], bs[i])
	}
	return nil
}

// ---------------------------------------------------------------- ordered folds

// FoldBatch does, for every i, dsts[i].Merge(s) for s in srcs[i] in order
// (same logic as host/crdt.hpp FoldBatch, tested on the GPU by tests/cpp/test_scenarios.cpp)
// (AWSet semantics, awset.go:103-161) in one call (crdt_awset_fold_batch).
func (e *Engine) FoldBatch(dsts []*crdt.AWSet, srcs [][]*crdt.AWSet) error {
	ds := make([]docState, len(dsts))
	ss := make([][]docState, len(srcs))
	for i, d := range dsts {
		ds[i] = stateOf(d, nil)
	}
	for i, l := range srcs {
		for _, s := range l {
			ss[i] = append(ss[i], stateOf(s, nil))
		}
	}
	return e.fold(false, dsts, ds, ss)
}

// DeltaMerge is dst.Merge(src) for AWSetDelta (awset-delta_test.go:51) on the GPU.
func (e *Engine) DeltaMerge(dst, src *AWSetDelta) error {
	return e.DeltaMergeBatch([]*AWSetDelta{dst}, [][]*AWSetDelta{{src}})
}

// (DeltaMergeBatch: same logic as host/crdt.hpp DeltaMergeBatch, tested on the GPU by
// tests/cpp/test_scenarios.cpp.)
// DeltaMergeBatch does, for every i, dsts[i].Merge(s) for s in srcs[i] in
// order (AWSetDelta semantics, awset-delta_test.go:51-166: the path select on
// Counter(src.Actor), MakeDeltaMergeData's pruning, the no-op that skips even
// the clock merge) in one call (crdt_awset_fold_batch, CRDT_FOLD_DELTA).
// dsts[i].Deleted is not changed (the reference's merges never touch it).
func (e *Engine) DeltaMergeBatch(dsts []*AWSetDelta, srcs [][]*AWSetDelta) error {
	ad := make([]*crdt.AWSet, len(dsts))
	ds := make([]docState, len(dsts))
	ss := make([][]docState, len(srcs))
	for i, d := range dsts {
		ad[i] = &d.AWSet
		ds[i] = stateOf(&d.AWSet, d.Deleted)
	}
	for i, l := range srcs {
		for _, s := range l {
			ss[i] = append(ss[i], stateOf(&s.AWSet, s.Deleted))
		}
	}
	return e.fold(true, ad, ds, ss)
}

func (e *Engine) fold(delta bool, dsts []*crdt.AWSet, ds []docState, ss [][]docState) error {
	if len(dsts) != len(ss) {
		return fmt.Errorf("fold: %d destinations, %d source lists", len(dsts), len(ss))
	}
	n := len(dsts)
	if n == 0 {
		return nil
	}
	if err := distinct(dsts); err != nil {
		return err
	}
	docs := make([][]docState, n)
	keys := make([]docKeys, n)
	widths := make([]int, n)
	ns, nent, ntomb := 0, 0, 0
	for i := range dsts {
		docs[i] = append([]docState{ds[i]}, ss[i]...)
		maps := []map[string]crdt.Dot{ds[i].Entries}
		for _, s := range ss[i] {
			maps = append(maps, s.Entries, s.Deleted)
			nent += len(s.Entries)
			ntomb += len(s.Deleted)
		}
		ns += len(ss[i])
		keys[i] = internDoc(maps...)
		widths[i] = foldWidth(delta, docs[i]) // from the snapshot, before any map changes
	}
	R, err := raggedChecks(delta, docs)
	if err != nil {
		return err
	}
	var a arena
	defer a.free()
	cd, doff := a.batch(dsts, keys, R)
	docSrcs, srcActor, svv := a.u32(n+1), a.u32(ns), a.u64(ns*R)
	eoff, ent := a.u32(ns+1), a.entries(nent)
	var toff []uint32
	var tomb entries
	if delta && ntomb > 0 {
		toff, tomb = a.u32(ns+1), a.entries(ntomb)
	}
	o := a.out(n, R, int(doff[n])+nent)
	if a.err != nil {
		return a.err
	}
	q, at, tat := 0, 0, 0
	for i := range dsts {
		docSrcs[i] = uint32(q)
		for _, s := range ss[i] {
			srcActor[q] = uint32(s.Actor)
			putVV(svv[q*R:(q+1)*R], s.VersionVector)
			eoff[q] = uint32(at)
			at = ent.put(at, s.Entries, keys[i])
			if toff != nil {
				toff[q] = uint32(tat)
				tat = tomb.put(tat, s.Deleted, keys[i])
			}
			q++
		}
	}
	docSrcs[n], eoff[ns] = uint32(ns), uint32(nent)
	cs := C.crdt_src_batch{n_docs: C.uint32_t(n), R: C.uint32_t(R), doc_srcs: p32(docSrcs),
		src_actor: p32(srcActor), vv: p64(svv), entry_off: p32(eoff), keys: p64(ent.keys),
		actors: p32(ent.actors), counters: p64(ent.counters)}
	if toff != nil {
		toff[ns] = uint32(ntomb)
		cs.tomb_off, cs.tkeys, cs.tactors, cs.tcounters = p32(toff), p64(tomb.keys), p32(tomb.actors), p64(tomb.counters)
	}
	mode := C.int(C.CRDT_FOLD_AWSET)
	if delta {
		mode = C.CRDT_FOLD_DELTA
	}
	if rc := C.crdt_awset_fold_batch(e.ctx, mode, &cd, &cs, &o.c); rc != 0 {
		return errOf("crdt_awset_fold_batch", rc)
	}
	for i, dst := range dsts {
		o.apply(i, R, widths[i], keys[i], dst)
	}
	return nil
}

// ---------------------------------------------------------------- delta extraction

// Delta is what one source state has to send a peer: Kind is CRDT_DELTA_NONE
// (nothing: skip it), CRDT_DELTA_DELTA or CRDT_DELTA_FULL (first contact), and
// State holds the entries and tombstones to ship with the source's actor and
// clock. The receiver merges State with DeltaMerge / DeltaMergeBatch.
type Delta struct {
	Kind  int
	State *AWSetDelta
}

// DeltaBatch is the sending side of anti-entropy: for every i and every state
// s of srcs[i], what a peer whose replica of document i has reached the clock
// peers[i] still needs of s -- MakeDeltaMergeData(peers[i])
// (awset-delta_test.go:79-105) or, at Counter(s.Actor) == 0, the whole state
// (:53) -- in one call (crdt_awset_delta_extract_batch). For any peers[i] at or
// below the receiver's real clock, merging the result equals merging the states.
// Clocks shorter than the longest one of the batch count as padded with zeros.
func (e *Engine) DeltaBatch(srcs [][]*AWSetDelta, peers []crdt.VersionVector) ([][]Delta, error) {
	if len(srcs) != len(peers) {
		return nil, fmt.Errorf("DeltaBatch: %d source lists, %d peer clocks", len(srcs), len(peers))
	}
	n := len(srcs)
	res := make([][]Delta, n)
	if n == 0 {
		return res, nil
	}
	keys := make([]docKeys, n)
	R, ns, nent, ntomb := 1, 0, 0, 0
	for i, l := range srcs {
		R = max(R, len(peers[i]))
		var maps []map[string]crdt.Dot
		for _, s := range l {
			R = max(R, len(s.VersionVector))
			maps = append(maps, s.Entries, s.Deleted)
			nent += len(s.Entries)
			ntomb += len(s.Deleted)
		}
		ns += len(l)
		keys[i] = internDoc(maps...)
	}
	var a arena
	defer a.free()
	docSrcs, srcActor, svv, pvv := a.u32(n+1), a.u32(ns), a.u64(ns*R), a.u64(n*R)
	eoff, ent, toff, tomb := a.u32(ns+1), a.entries(nent), a.u32(ns+1), a.entries(ntomb)
	oDocSrcs, oActor, ovv := a.u32(n+1), a.u32(ns), a.u64(ns*R)
	oeoff, oent, otoff, otomb := a.u32(ns+1), a.entries(nent), a.u32(ns+1), a.entries(ntomb)
	kind := a.u32((ns + 3) / 4) // ns bytes
	if a.err != nil {
		return nil, a.err
	}
	q, at, tat := 0, 0, 0
	for i, l := range srcs {
		docSrcs[i] = uint32(q)
		putVV(pvv[i*R:(i+1)*R], peers[i])
		for _, s := range l {
			srcActor[q] = uint32(s.Actor)
			putVV(svv[q*R:(q+1)*R], s.VersionVector)
			eoff[q], toff[q] = uint32(at), uint32(tat)
			at = ent.put(at, s.Entries, keys[i])
			tat = tomb.put(tat, s.Deleted, keys[i])
			q++
		}
	}
	docSrcs[n], eoff[ns], toff[ns] = uint32(ns), uint32(nent), uint32(ntomb)
	cs := C.crdt_src_batch{n_docs: C.uint32_t(n), R: C.uint32_t(R), doc_srcs: p32(docSrcs),
		src_actor: p32(srcActor), vv: p64(svv), entry_off: p32(eoff), keys: p64(ent.keys),
		actors: p32(ent.actors), counters: p64(ent.counters), tomb_off: p32(toff), tkeys: p64(tomb.keys),
		tactors: p32(tomb.actors), tcounters: p64(tomb.counters)}
	dout := C.crdt_delta_out{doc_srcs: p32(oDocSrcs), src_actor: p32(oActor), vv: p64(ovv), entry_off: p32(oeoff),
		keys: p64(oent.keys), actors: p32(oent.actors), counters: p64(oent.counters), tomb_off: p32(otoff),
		tkeys: p64(otomb.keys), tactors: p32(otomb.actors), tcounters: p64(otomb.counters),
		kind: (*C.uint8_t)(unsafe.Pointer(unsafe.SliceData(kind)))}
	if rc := C.crdt_awset_delta_extract_batch(e.ctx, &cs, p64(pvv), &dout); rc != 0 {
		return nil, errOf("crdt_awset_delta_extract_batch", rc)
	}
	kinds := unsafe.Slice((*uint8)(unsafe.Pointer(unsafe.SliceData(kind))), ns)
	dots := func(es entries, lo, hi uint32, ks docKeys) map[string]crdt.Dot {
		if lo == hi {
			return nil
		}
		m := make(map[string]crdt.Dot, hi-lo)
		for j := lo; j < hi; j++ {
			m[ks[es.keys[j]]] = crdt.Dot{Actor: crdt.Actor(es.actors[j]), Counter: uint(es.counters[j])}
		}
		return m
	}
	q = 0
	for i, l := range srcs {
		res[i] = make([]Delta, len(l))
		for j, s := range l {
			st := &AWSetDelta{AWSet: crdt.AWSet{Actor: s.Actor}}
			st.VersionVector = append(crdt.VersionVector(nil), s.VersionVector...)
			st.Entries = dots(oent, oeoff[q], oeoff[q+1], keys[i])
			if st.Entries == nil {
				st.Entries = map[string]crdt.Dot{}
			}
			st.Deleted = dots(otomb, otoff[q], otoff[q+1], keys[i])
			res[i][j] = Delta{Kind: int(kinds[q]), State: st}
			q++
		}
	}
	return res, nil
}

// ---------------------------------------------------------------- resident replicas

// Replica is one device-resident replica of every document of a batch: the
// state batch an apply, join, exchange, fold or scatter call wrote (State, as it
// stands: offsets, counts, slack), its AWSetDelta.Deleted (Tombs, nil: none) and
// its actor -- DocActor, a device array of one actor per document, or Actor for
// every document when DocActor is nil. Every pointer in State and Tombs is a
// device pointer.
type Replica struct {
	State    C.crdt_awset_batch
	Tombs    *C.crdt_tomb_batch
	DocActor *C.uint32_t
	Actor    uint32
}

// SourcesBatch gathers resident replicas, in fold order, into the packed source
// batch `out` on the device (crdt_awset_sources_async): source d*len(reps)+p is
// replica p's document d, live entries and tombstones only. out (device arrays,
// entrySlots entries and tombSlots tombstones) is then the srcs of a fold or a
// delta extraction as it stands. The call is asynchronous on stream; device-side
// errors (a total above the slots) surface at the context's next sync.
func (e *Engine) SourcesBatch(reps []Replica, entrySlots, tombSlots uint32, out *C.crdt_delta_out,
	stream unsafe.Pointer) error {
	if len(reps) == 0 || len(reps) > C.CRDT_MAX_REPLICAS {
		return fmt.Errorf("SourcesBatch: %d replicas (1..%d)", len(reps), int(C.CRDT_MAX_REPLICAS))
	}
	// the descriptors and the structs they point at live in C memory for the call
	var a arena
	defer a.free()
	crSize, stSize := int(unsafe.Sizeof(C.crdt_replica{})), int(unsafe.Sizeof(C.crdt_awset_batch{}))
	tbSize := int(unsafe.Sizeof(C.crdt_tomb_batch{}))
	pr, ps, pt := a.alloc(len(reps)*crSize), a.alloc(len(reps)*stSize), a.alloc(len(reps)*tbSize)
	if a.err != nil {
		return a.err
	}
	crs := unsafe.Slice((*C.crdt_replica)(pr), len(reps))
	sts := unsafe.Slice((*C.crdt_awset_batch)(ps), len(reps))
	tbs := unsafe.Slice((*C.crdt_tomb_batch)(pt), len(reps))
	for i, r := range reps {
		sts[i] = r.State
		cr := C.crdt_replica{state: &sts[i], doc_actor: r.DocActor, actor: C.uint32_t(r.Actor)}
		if r.Tombs != nil {
			tbs[i] = *r.Tombs
			cr.tombs = &tbs[i]
		}
		crs[i] = cr
	}
	if rc := C.crdt_awset_sources_async(e.ctx, &crs[0], C.uint32_t(len(reps)), C.uint32_t(entrySlots),
		C.uint32_t(tombSlots), out, stream); rc != 0 {
		return errOf("crdt_awset_sources_async", rc)
	}
	return nil
}

// ReplicaOut is the device storage a replica select or scatter writes: the state
// (StateOut), the tombstones (Tombs, nil: none -- allowed only when no input replica
// has Tombs) and one actor per output document (DocActor, nil: not written).
// Every pointer is a device pointer.
type ReplicaOut struct {
	StateOut C.crdt_awset_out
	Tombs    *C.crdt_tomb_out
	DocActor *C.uint32_t
}

// replicaC lays a Replica out in C memory for the length of one call.
func replicaC(a *arena, r *Replica) *C.crdt_replica {
	pr := a.alloc(int(unsafe.Sizeof(C.crdt_replica{})))
	ps := a.alloc(int(unsafe.Sizeof(C.crdt_awset_batch{})))
	pt := a.alloc(int(unsafe.Sizeof(C.crdt_tomb_batch{})))
	if a.err != nil {
		return nil
	}
	st := (*C.crdt_awset_batch)(ps)
	*st = r.State
	cr := C.crdt_replica{state: st, doc_actor: r.DocActor, actor: C.uint32_t(r.Actor)}
	if r.Tombs != nil {
		tb := (*C.crdt_tomb_batch)(pt)
		*tb = *r.Tombs
		cr.tombs = tb
	}
	out := (*C.crdt_replica)(pr)
	*out = cr
	return out
}

// replicaOutC lays a ReplicaOut out in C memory for the length of one call.
func replicaOutC(a *arena, o *ReplicaOut) *C.crdt_replica_out {
	po := a.alloc(int(unsafe.Sizeof(C.crdt_replica_out{})))
	ps := a.alloc(int(unsafe.Sizeof(C.crdt_awset_out{})))
	pt := a.alloc(int(unsafe.Sizeof(C.crdt_tomb_out{})))
	if a.err != nil {
		return nil
	}
	st := (*C.crdt_awset_out)(ps)
	*st = o.StateOut
	co := C.crdt_replica_out{state: st, doc_actor: o.DocActor}
	if o.Tombs != nil {
		tb := (*C.crdt_tomb_out)(pt)
		*tb = *o.Tombs
		co.tombs = tb
	}
	out := (*C.crdt_replica_out)(po)
	*out = co
	return out
}

// ReplicaSelect gathers documents idx[0..*nIdx) of a resident replica (idx nil:
// the identity; nIdx nil: nOut) into `out` on the device, with their
// AWSetDelta.Deleted and their actors, entries and tombstones each packed with
// no slack (crdt_replica_select_async). idx and nIdx are device pointers: a
// compare or digest worklist and its n_work feed the call with nothing read
// back. With idx and nIdx nil and nOut the replica's document count it compacts
// the replica. Asynchronous on stream; device-side errors surface at the
// context's next sync.
func (e *Engine) ReplicaSelect(rep *Replica, idx, nIdx *C.uint32_t, nOut, entrySlots, tombSlots uint32,
	out *ReplicaOut, stream unsafe.Pointer) error {
	var a arena
	defer a.free()
	cr, co := replicaC(&a, rep), replicaOutC(&a, out)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_replica_select_async(e.ctx, cr, idx, nIdx, C.uint32_t(nOut), C.uint32_t(entrySlots),
		C.uint32_t(tombSlots), co, stream); rc != 0 {
		return errOf("crdt_replica_select_async", rc)
	}
	return nil
}

// ReplicaScatter puts a sub-replica back into the resident replica it was
// selected from (crdt_replica_scatter_async): document d of out is sub's document
// j when idx[j] == d for some j < *nIdx, and rep's document d otherwise, with its
// tombstones and its actor. sub is typically the output of a delta exchange or an
// apply over the selected documents. Asynchronous on stream; device-side errors
// surface at the context's next sync.
func (e *Engine) ReplicaScatter(rep, sub *Replica, idx, nIdx *C.uint32_t, entrySlots, tombSlots uint32,
	out *ReplicaOut, stream unsafe.Pointer) error {
	var a arena
	defer a.free()
	cr, cs, co := replicaC(&a, rep), replicaC(&a, sub), replicaOutC(&a, out)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_replica_scatter_async(e.ctx, cr, cs, idx, nIdx, C.uint32_t(entrySlots),
		C.uint32_t(tombSlots), co, stream); rc != 0 {
		return errOf("crdt_replica_scatter_async", rc)
	}
	return nil
}

// ReplicaInPlace is a device-resident replica updated in place: the state's
// arrays with its counts (StateOut; every array but the offsets is written), its
// tombstones with their counts (Tombs, nil: the replica keeps none) and one actor
// per document (DocActor, nil: actors not written). Every pointer is a device
// pointer.
type ReplicaInPlace struct {
	StateOut C.crdt_awset_out
	NDocs, R uint32
	Tombs    *C.crdt_tomb_out
	DocActor *C.uint32_t
}

// SpillOut receives the sub documents an in-place scatter could not place:
// SpillJ their indices in sub, ascending, SpillDoc the replica document each
// names, NSpill their number (one device word). Each list holds as many words as
// sub has documents.
type SpillOut struct {
	SpillJ, SpillDoc, NSpill *C.uint32_t
}

// ReplicaScatterInPlace writes each document of sub into the slots its replica
// document idx[j] already owns when its live entries and tombstones fit them,
// and lists it in spill otherwise (crdt_replica_scatter_inplace_async). Nothing
// else of rep is touched: no packed copy of the replica is made, which is what
// ReplicaScatter costs. ReplicaSelect(sub, spill.SpillJ, spill.NSpill, ..)
// followed by ReplicaScatter(rep, that, spill.SpillDoc, spill.NSpill, ..) puts
// the spilled documents back. Asynchronous on stream; device-side errors surface
// at the context's next sync.
func (e *Engine) ReplicaScatterInPlace(rep *ReplicaInPlace, sub *Replica, idx, nIdx *C.uint32_t, spill *SpillOut,
	stream unsafe.Pointer) error {
	var a arena
	defer a.free()
	cs := replicaC(&a, sub)
	pr := a.alloc(int(unsafe.Sizeof(C.crdt_replica_inplace{})))
	pp := a.alloc(int(unsafe.Sizeof(C.crdt_spill_out{})))
	if a.err != nil {
		return a.err
	}
	ri := C.crdt_replica_inplace{n_docs: C.uint32_t(rep.NDocs), R: C.uint32_t(rep.R), offsets: rep.StateOut.offsets,
		counts: rep.StateOut.counts, keys: rep.StateOut.keys, actors: rep.StateOut.actors, counters: rep.StateOut.counters,
		vv: rep.StateOut.vv, doc_actor: rep.DocActor}
	if rep.Tombs != nil {
		ri.tomb_offsets, ri.tomb_counts = rep.Tombs.offsets, rep.Tombs.counts
		ri.tkeys, ri.tactors, ri.tcounters = rep.Tombs.keys, rep.Tombs.actors, rep.Tombs.counters
	}
	sp := C.crdt_spill_out{spill_j: spill.SpillJ, spill_doc: spill.SpillDoc, n_spill: spill.NSpill}
	*(*C.crdt_replica_inplace)(pr) = ri
	*(*C.crdt_spill_out)(pp) = sp
	if rc := C.crdt_replica_scatter_inplace_async(e.ctx, (*C.crdt_replica_inplace)(pr), cs, idx, nIdx,
		(*C.crdt_spill_out)(pp), stream); rc != 0 {
		return errOf("crdt_replica_scatter_inplace_async", rc)
	}
	return nil
}

// Headroom is the layout policy of ReplicaRepack (crdt_headroom): a document with
// n live slots owns round_up(n + max(MinSpare, (n*Num)>>Shift), Align) slots.
// Align is a power of two from 1 to 64 and Shift at most 31. A nil *Headroom is
// the packed layout.
type Headroom struct {
	MinSpare, Num, Shift, Align uint32
}

func headroomC(a *arena, h *Headroom) *C.crdt_headroom {
	if h == nil {
		return nil
	}
	ph := a.alloc(int(unsafe.Sizeof(C.crdt_headroom{})))
	if a.err != nil {
		return nil
	}
	ch := C.crdt_headroom{min_spare: C.uint32_t(h.MinSpare), num: C.uint32_t(h.Num), shift: C.uint32_t(h.Shift),
		align: C.uint32_t(h.Align)}
	*(*C.crdt_headroom)(ph) = ch
	return (*C.crdt_headroom)(ph)
}

// Capacity is the slot count the policy gives a document with n live slots
// (crdt_headroom_capacity): the library's own expression, saturated at 2^32 - 1.
func (h *Headroom) Capacity(n uint32) uint32 {
	if h == nil {
		return uint32(C.crdt_headroom_capacity(nil, C.uint32_t(n)))
	}
	ch := C.crdt_headroom{min_spare: C.uint32_t(h.MinSpare), num: C.uint32_t(h.Num), shift: C.uint32_t(h.Shift),
		align: C.uint32_t(h.Align)}
	return uint32(C.crdt_headroom_capacity(&ch, C.uint32_t(n)))
}

// ReplicaRepack is ReplicaSelect (sub nil) or ReplicaScatter (sub given; nOut must
// be rep's document count) writing a layout with spare slots
// (crdt_replica_repack_async): document j of out owns entryRoom.Capacity(live
// entries) entry slots and tombRoom.Capacity(live tombstones) tombstone slots, the
// offsets are the prefix of those capacities, the counts are the live counts, and
// no slot at or past a live count is written. out is a replica as it stands and a
// ReplicaInPlace target with no copy, so a replica that has spilled regains the
// room ReplicaScatterInPlace needs. Asynchronous on stream; device-side errors
// surface at the context's next sync.
func (e *Engine) ReplicaRepack(rep, sub *Replica, idx, nIdx *C.uint32_t, nOut uint32, entryRoom, tombRoom *Headroom,
	entrySlots, tombSlots uint32, out *ReplicaOut, stream unsafe.Pointer) error {
	var a arena
	defer a.free()
	cr, co := replicaC(&a, rep), replicaOutC(&a, out)
	var cs *C.crdt_replica
	if sub != nil {
		cs = replicaC(&a, sub)
	}
	er, tr := headroomC(&a, entryRoom), headroomC(&a, tombRoom)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_replica_repack_async(e.ctx, cr, cs, idx, nIdx, C.uint32_t(nOut), er, tr, C.uint32_t(entrySlots),
		C.uint32_t(tombSlots), co, stream); rc != 0 {
		return errOf("crdt_replica_repack_async", rc)
	}
	return nil
}

// ---------------------------------------------------------------- logged join

// MergeLog is the device storage a logged join writes beside the merged state
// (crdt_merge_log): per document the dst entries the merge removed, in dst's slot
// layout, and the src entries it added or moved a common key to, in src's, with
// the CRDT_DIFF_* flags and the summary. Every pointer is a device pointer;
// summary and ups_kind may be nil.
type MergeLog struct {
	Log C.crdt_merge_log
}

// JoinLog is crdt_awset_join_async with the merge's decision log
// (awset.go:109-158) written beside the merged state from the same read
// (crdt_awset_join_log_async): out holds what the join writes; log's removed list
// of document d starts at dst.offsets[d], its upserted list at src.offsets[d].
// dst, src, out and log name device arrays. Asynchronous on stream; device-side
// errors surface at the context's next sync.
func (e *Engine) JoinLog(dst, src *C.crdt_awset_batch, out *C.crdt_awset_out, log *MergeLog,
	stream unsafe.Pointer) error {
	if dst == nil || src == nil || out == nil || log == nil {
		return fmt.Errorf("JoinLog: nil argument")
	}
	if rc := C.crdt_awset_join_log_async(e.ctx, dst, src, out, &log.Log, stream); rc != 0 {
		return errOf("crdt_awset_join_log_async", rc)
	}
	return nil
}

// ExchangeLog is crdt_awset_exchange_async with both directions' logs, from one
// read of both states (crdt_awset_exchange_log_async): logAB's removed list is in
// a's layout and its upserted list in b's, logBA's the other way round. The two
// outputs share no array, the key column included.
func (e *Engine) ExchangeLog(a, b *C.crdt_awset_batch, outAB, outBA *C.crdt_awset_out, logAB, logBA *MergeLog,
	stream unsafe.Pointer) error {
	if a == nil || b == nil || outAB == nil || outBA == nil || logAB == nil || logBA == nil {
		return fmt.Errorf("ExchangeLog: nil argument")
	}
	if rc := C.crdt_awset_exchange_log_async(e.ctx, a, b, outAB, outBA, &logAB.Log, &logBA.Log, stream); rc != 0 {
		return errOf("crdt_awset_exchange_log_async", rc)
	}
	return nil
}

// FoldLog is crdt_awset_fold_async with the log of the whole ordered fold written
// beside the merged state (crdt_awset_fold_log_async): out holds what the fold
// writes; log's removed list of document d starts at dst.offsets[d], its upserted
// list at entry_off[doc_srcs[d]] with the document's source entry slots for
// capacity. The log is the fold's net effect, crdt_awset_diff_async(dst, out)'s
// answer: steps in between do not show. mode is C.CRDT_FOLD_AWSET or
// C.CRDT_FOLD_DELTA; the receiver of a delta message gets its index updates from
// this call. Asynchronous on stream; device-side errors surface at the context's
// next sync.
func (e *Engine) FoldLog(mode int, dst *C.crdt_awset_batch, srcs *C.crdt_src_batch, out *C.crdt_awset_out,
	log *MergeLog, stream unsafe.Pointer) error {
	if dst == nil || srcs == nil || out == nil || log == nil {
		return fmt.Errorf("FoldLog: nil argument")
	}
	if rc := C.crdt_awset_fold_log_async(e.ctx, C.int(mode), dst, srcs, out, &log.Log, stream); rc != 0 {
		return errOf("crdt_awset_fold_log_async", rc)
	}
	return nil
}

// ApplyLog is crdt_awset_apply_async (batched Add / Del / AWSetDelta.Del on resident
// documents) with the log of what the ops changed written beside the new state
// (crdt_awset_apply_log_async): out and tombOut hold what the plain call writes;
// log's removed list of document d starts at state.offsets[d] and holds the state
// entries the ops removed with the dot they had, its upserted list starts at
// ops.op_off[d] and holds the entries an Add left new (CRDT_DIFF_ADDED) or under
// another dot (CRDT_DIFF_UPDATED). The log is crdt_awset_diff_async(state, out)'s
// answer; tombstone changes are not part of it. A refused document's log is empty.
// tombs and tombOut may be nil as in the plain call. With JoinLog and FoldLog an
// index beside a replica follows local ops and merges alike. Asynchronous on
// stream; device-side errors surface at the context's next sync.
func (e *Engine) ApplyLog(state *C.crdt_awset_batch, tombs *C.crdt_tomb_batch, ops *C.crdt_op_batch,
	out *C.crdt_awset_out, tombOut *C.crdt_tomb_out, log *MergeLog, stream unsafe.Pointer) error {
	if state == nil || ops == nil || out == nil || log == nil {
		return fmt.Errorf("ApplyLog: nil argument")
	}
	if rc := C.crdt_awset_apply_log_async(e.ctx, state, tombs, ops, out, tombOut, &log.Log, stream); rc != 0 {
		return errOf("crdt_awset_apply_log_async", rc)
	}
	return nil
}

// ---------------------------------------------------------------- delta merge of a resident pair

// DeltaJoin is (*AWSetDelta).Merge on resident replicas as they stand
// (crdt_awset_delta_join_async): out[d] = dst[d] <- src[d], in the join's layout.
// dst is a plain state (the destination's tombstones and actor are not read); kind,
// a device array of one byte per document or nil, receives CRDT_DELTA_FULL / DELTA /
// NONE. Asynchronous on stream; device-side errors surface at the context's next sync.
func (e *Engine) DeltaJoin(dst *C.crdt_awset_batch, src *Replica, out *C.crdt_awset_out, kind *C.uint8_t,
	stream unsafe.Pointer) error {
	if dst == nil || src == nil || out == nil {
		return fmt.Errorf("DeltaJoin: nil argument")
	}
	var a arena
	defer a.free()
	cs := replicaC(&a, src)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_awset_delta_join_async(e.ctx, dst, cs, out, kind, stream); rc != 0 {
		return errOf("crdt_awset_delta_join_async", rc)
	}
	return nil
}

// DeltaExchange is both delta merges of a resident pair from one read of both
// (crdt_awset_delta_exchange_async): outAB = a <- b and outBA = b <- a. kindAB and
// kindBA are device arrays of one byte per document, or nil.
func (e *Engine) DeltaExchange(ra, rb *Replica, outAB, outBA *C.crdt_awset_out, kindAB, kindBA *C.uint8_t,
	stream unsafe.Pointer) error {
	if ra == nil || rb == nil || outAB == nil || outBA == nil {
		return fmt.Errorf("DeltaExchange: nil argument")
	}
	var a arena
	defer a.free()
	ca, cb := replicaC(&a, ra), replicaC(&a, rb)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_awset_delta_exchange_async(e.ctx, ca, cb, outAB, outBA, kindAB, kindBA, stream); rc != 0 {
		return errOf("crdt_awset_delta_exchange_async", rc)
	}
	return nil
}

// DeltaJoinLog is DeltaJoin with the merge's decision log written beside the merged
// state from the same read (crdt_awset_delta_join_log_async): log's removed list of
// document d starts at dst.offsets[d], its upserted list at src's offsets[d]. A NONE
// document has empty lists and flags 0; a common key that the delta merge moves to
// src's dot and a tombstone then removes is recorded as removed with dst's dot.
func (e *Engine) DeltaJoinLog(dst *C.crdt_awset_batch, src *Replica, out *C.crdt_awset_out, kind *C.uint8_t,
	log *MergeLog, stream unsafe.Pointer) error {
	if dst == nil || src == nil || out == nil || log == nil {
		return fmt.Errorf("DeltaJoinLog: nil argument")
	}
	var a arena
	defer a.free()
	cs := replicaC(&a, src)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_awset_delta_join_log_async(e.ctx, dst, cs, out, kind, &log.Log, stream); rc != 0 {
		return errOf("crdt_awset_delta_join_log_async", rc)
	}
	return nil
}

// DeltaExchangeLog is DeltaExchange with both directions' logs
// (crdt_awset_delta_exchange_log_async): logAB's removed list is in a's layout and
// its upserted list in b's, logBA's the other way round.
func (e *Engine) DeltaExchangeLog(ra, rb *Replica, outAB, outBA *C.crdt_awset_out, kindAB, kindBA *C.uint8_t,
	logAB, logBA *MergeLog, stream unsafe.Pointer) error {
	if ra == nil || rb == nil || outAB == nil || outBA == nil || logAB == nil || logBA == nil {
		return fmt.Errorf("DeltaExchangeLog: nil argument")
	}
	var a arena
	defer a.free()
	ca, cb := replicaC(&a, ra), replicaC(&a, rb)
	if a.err != nil {
		return a.err
	}
	if rc := C.crdt_awset_delta_exchange_log_async(e.ctx, ca, cb, outAB, outBA, kindAB, kindBA, &logAB.Log,
		&logBA.Log, stream); rc != 0 {
		return errOf("crdt_awset_delta_exchange_log_async", rc)
	}
	return nil
}

// ---------------------------------------------------------------- state digests

// HostBatch is a packed batch in host memory: State as arena.batch lays it out
// (or any crdt_awset_batch over host arrays; a document's entries may lie in any
// order, so a map can be packed in iteration order) and its AWSetDelta.Deleted
// (Tombs, nil: none).
type HostBatch struct {
	State C.crdt_awset_batch
	Tombs *C.crdt_tomb_batch
}

// Digest is the 16-byte state digest of every document (crdt_awset_digest_host,
// no GPU): [d][0] covers the element set, [d][1] elements, dots, Deleted and
// clock. A peer compares these with the digests a device computed
// (crdt_awset_digest_async) to find the documents that differ, provided both
// share the key interning.
func (b *HostBatch) Digest() ([][2]uint64, error) {
	n := int(b.State.n_docs)
	flat := make([]uint64, 2*n+2)
	if rc := C.crdt_awset_digest_host(&b.State, b.Tombs, p64(flat)); rc != 0 {
		return nil, errOf("crdt_awset_digest_host", rc)
	}
	out := make([][2]uint64, n)
	for d := range out {
		out[d] = [2]uint64{flat[2*d], flat[2*d+1]}
	}
	return out, nil
}

// Digest modes of DigestIdx.
const (
	DigestGather = uint32(C.CRDT_DIGEST_GATHER) // document idx[j] of state -> digest[2*idx[j]], [2*idx[j]+1]
	DigestPlace  = uint32(C.CRDT_DIGEST_PLACE)  // document j of state (a sub-batch) -> the same words
)

// DigestIdx re-digests only the documents a device worklist names
// (crdt_awset_digest_idx_async) and writes their two words into digest, the
// resident array of nDigestDocs documents, at their own positions; every other
// word keeps its bits. DigestGather: state (and tombs) is the resident replica
// and nDigestDocs its document count. DigestPlace: state is a sub-batch of at
// least nMax documents whose document j is the replica's document idx[j]; a
// target named twice is the caller's error and is not checked. idx, nIdx and
// digest are device pointers; nIdx may be nil (nMax documents), tombs may be nil.
// Asynchronous on stream; device-side errors surface at the context's next sync.
func (e *Engine) DigestIdx(state *C.crdt_awset_batch, tombs *C.crdt_tomb_batch, idx, nIdx *C.uint32_t,
	nMax, nDigestDocs, mode uint32, digest *C.uint64_t, stream unsafe.Pointer) error {
	if state == nil || idx == nil || digest == nil {
		return fmt.Errorf("DigestIdx: nil argument")
	}
	if rc := C.crdt_awset_digest_idx_async(e.ctx, state, tombs, idx, nIdx, C.uint32_t(nMax), C.uint32_t(nDigestDocs),
		C.uint32_t(mode), digest, stream); rc != 0 {
		return errOf("crdt_awset_digest_idx_async", rc)
	}
	return nil
}

// DigestTreeFanout is the fan-out of the digest tree: one node covers 16 children.
const DigestTreeFanout = uint32(C.CRDT_DIGEST_TREE_FANOUT)

// DigestTreeLayout is the shape of the digest tree over nDocs documents
// (crdt_digest_tree_layout): L levels above the digest array, Nodes[l] nodes on
// level l (Nodes[0] = nDocs) and Off[l] the node offset of level l >= 1 in the
// tree array, which holds two words per node.
type DigestTreeLayout struct {
	L     int
	Nodes [9]uint32
	Off   [9]uint32
}

// TreeLayout computes the layout on the host.
func TreeLayout(nDocs uint32) DigestTreeLayout {
	var t DigestTreeLayout
	var nodes, off [9]C.uint32_t
	t.L = int(C.crdt_digest_tree_layout(C.uint32_t(nDocs), &nodes[0], &off[0]))
	for l := range nodes {
		t.Nodes[l], t.Off[l] = uint32(nodes[l]), uint32(off[l])
	}
	return t
}

// TreeWords is the length of the tree array in uint64 words.
func (t DigestTreeLayout) TreeWords() int {
	if t.L == 0 {
		return 0
	}
	return 2 * (int(t.Off[t.L]) + 1)
}

// DigestTreeHost builds the digest tree of a host digest array (two words per
// document, as Digest returns them flattened) without a GPU
// (crdt_digest_tree_host): levels 1 .. L concatenated, two words per node.
func DigestTreeHost(digest []uint64) ([]uint64, error) {
	n := uint32(len(digest) / 2)
	tree := make([]uint64, TreeLayout(n).TreeWords()+2)
	if n == 0 {
		return tree[:0], nil
	}
	if rc := C.crdt_digest_tree_host(p64(digest), C.uint32_t(n), p64(tree)); rc != 0 {
		return nil, errOf("crdt_digest_tree_host", rc)
	}
	return tree[:len(tree)-2], nil
}

// DigestTree builds every level of the tree over a device digest array
// (crdt_digest_tree_async). digest and tree are device pointers; the tree is
// rebuilt whole from the array, which DigestIdx keeps current. Asynchronous on
// stream.
func (e *Engine) DigestTree(digest *C.uint64_t, nDocs uint32, tree *C.uint64_t, stream unsafe.Pointer) error {
	if rc := C.crdt_digest_tree_async(e.ctx, digest, C.uint32_t(nDocs), tree, stream); rc != 0 {
		return errOf("crdt_digest_tree_async", rc)
	}
	return nil
}

// DigestTreeChildren is the sender's side of a descent
// (crdt_digest_tree_children_async): both words of the 16 children of every
// listed parent packed into out, 32 words per parent, zeros past the level.
// level is the node array the children lie in (the digest array, or the tree at
// 2*Off[l-1]) and nLevel its node count. parents and nParents are device
// pointers; parents nil is the identity, nParents nil means nMax. Asynchronous
// on stream; device-side errors surface at the context's next sync.
func (e *Engine) DigestTreeChildren(level *C.uint64_t, nLevel uint32, parents, nParents *C.uint32_t, nMax uint32,
	out *C.uint64_t, stream unsafe.Pointer) error {
	if out == nil {
		return fmt.Errorf("DigestTreeChildren: nil argument")
	}
	if rc := C.crdt_digest_tree_children_async(e.ctx, level, C.uint32_t(nLevel), parents, nParents, C.uint32_t(nMax),
		out, stream); rc != 0 {
		return errOf("crdt_digest_tree_children_async", rc)
	}
	return nil
}

// DigestTreeDiff is the receiver's side (crdt_digest_tree_diff_async): the
// listed parents' children of its own level against theirs, the peer's packed
// children for the same list. The children with flag & mask go to idxOut,
// ascending, their flags to flagsOut (may be nil) and their exact number to
// nOut; summary (may be nil) gets five counts. leaf: the children are documents
// and the flags are those of the digest comparison; otherwise bit 0 is "word 0
// differs" and bit 1 "word 1 differs". idxOut and nOut are the parents and
// nParents of the next level's two calls. All pointers are device pointers.
// Asynchronous on stream; device-side errors surface at the context's next sync.
func (e *Engine) DigestTreeDiff(mineLevel *C.uint64_t, nLevel uint32, theirs *C.uint64_t, parents, nParents *C.uint32_t,
	nMax uint32, leaf bool, mask uint32, idxOut *C.uint32_t, flagsOut *C.uint8_t, nOut *C.uint32_t, outMax uint32,
	summary *C.uint32_t, stream unsafe.Pointer) error {
	if idxOut == nil || nOut == nil {
		return fmt.Errorf("DigestTreeDiff: nil argument")
	}
	isLeaf := C.uint32_t(0)
	if leaf {
		isLeaf = 1
	}
	if rc := C.crdt_digest_tree_diff_async(e.ctx, mineLevel, C.uint32_t(nLevel), theirs, parents, nParents,
		C.uint32_t(nMax), isLeaf, C.uint32_t(mask), idxOut, flagsOut, nOut, C.uint32_t(outMax), summary,
		stream); rc != 0 {
		return errOf("crdt_digest_tree_diff_async", rc)
	}
	return nil
}

// ---------------------------------------------------------------- merge diff

// DocDiff is what turns one document's `before` into its `after`: merge's
// decision log (awset.go:109-158) in structured form. Removed holds the entries
// of before whose key after no longer has, with the dot they had; Added the
// entries of after under a key before did not have; Updated the entries of after
// whose key before had under another dot. Deleting Removed from before and then
// assigning Added and Updated gives after. Clock: the version vectors differ.
type DocDiff struct {
	Removed map[string]crdt.Dot
	Added   map[string]crdt.Dot
	Updated map[string]crdt.Dot
	Clock   bool
}

// DiffBatch computes DocDiff of (before[i], after[i]) for every i in one call
// (crdt_awset_diff_batch): both batches go up, only the two lists, their offsets
// and a flag byte per document come back. The lists are sized for the worst case
// (every entry of before removed, every entry of after upserted), so one call
// suffices. It reads the states and changes neither.
func (e *Engine) DiffBatch(before, after []*crdt.AWSet) ([]DocDiff, error) {
	if len(before) != len(after) {
		return nil, fmt.Errorf("DiffBatch: %d and %d states", len(before), len(after))
	}
	n := len(before)
	if n == 0 {
		return nil, nil
	}
	keys := make([]docKeys, n)
	R := 1
	for i := range before {
		keys[i] = internDoc(before[i].Entries, after[i].Entries)
		R = max(R, len(before[i].VersionVector), len(after[i].VersionVector))
	}
	var a arena
	defer a.free()
	cb, boff := a.batch(before, keys, R)
	ca, aoff := a.batch(after, keys, R)
	nr, nu := int(boff[n]), int(aoff[n])
	flags := a.u32((n + 3) / 4) // one byte per document
	remOff, upsOff := a.u32(n+1), a.u32(n+1)
	rem, ups := a.entries(nr+1), a.entries(nu+1)
	kind := a.u32((nu + 3) / 4) // one byte per upsert
	if a.err != nil {
		return nil, a.err
	}
	cdiff := C.crdt_diff_out{flags: (*C.uint8_t)(unsafe.Pointer(p32(flags))),
		rem_off: p32(remOff), rem_keys: p64(rem.keys), rem_actors: p32(rem.actors), rem_counters: p64(rem.counters),
		ups_off: p32(upsOff), ups_keys: p64(ups.keys), ups_actors: p32(ups.actors), ups_counters: p64(ups.counters),
		ups_kind: (*C.uint8_t)(unsafe.Pointer(p32(kind)))}
	if rc := C.crdt_awset_diff_batch(e.ctx, &cb, &ca, C.uint32_t(nr), C.uint32_t(nu), &cdiff); rc != 0 {
		return nil, errOf("crdt_awset_diff_batch", rc)
	}
	flagOf := unsafe.Slice((*uint8)(unsafe.Pointer(unsafe.SliceData(flags))), n)
	kindOf := unsafe.Slice((*uint8)(unsafe.Pointer(unsafe.SliceData(kind))), nu+1)
	res := make([]DocDiff, n)
	for d := range res {
		r := DocDiff{Removed: map[string]crdt.Dot{}, Added: map[string]crdt.Dot{}, Updated: map[string]crdt.Dot{},
			Clock: flagOf[d]&uint8(C.CRDT_DIFF_CLOCK) != 0}
		for j := remOff[d]; j < remOff[d+1]; j++ {
			r.Removed[keys[d][rem.keys[j]]] = crdt.Dot{Actor: crdt.Actor(rem.actors[j]), Counter: uint(rem.counters[j])}
		}
		for j := upsOff[d]; j < upsOff[d+1]; j++ {
			dot := crdt.Dot{Actor: crdt.Actor(ups.actors[j]), Counter: uint(ups.counters[j])}
			if kindOf[j] == uint8(C.CRDT_DIFF_UPDATED) {
				r.Updated[keys[d][ups.keys[j]]] = dot
			} else {
				r.Added[keys[d][ups.keys[j]]] = dot
			}
		}
		res[d] = r
	}
	return res, nil
}

// foldWidth is len(dst.VersionVector) after the fold, replayed on the clocks
// alone: every AWSet step merges the clock; a delta step merges it unless it
// is the no-op (awset-delta_test.go:60): Counter(src.Actor) != 0 (:53) and
// MakeDeltaMergeData finds no changed entry and no tombstone (:79-105). It
// runs after raggedChecks would have refused a batch that panics in Go.
func foldWidth(delta bool, doc []docState) int {
	V := append(crdt.VersionVector(nil), doc[0].VersionVector...)
	for _, s := range doc[1:] {
		if delta && counterOf(V, s.Actor) != 0 {
			brings := len(deletedOf(s)) > 0
			for _, d := range s.Entries {
				if !hasDotOf(V, d) {
					brings = true
					break
				}
			}
			if !brings {
				continue
			}
		}
		V.Merge(s.VersionVector)
	}
	return len(V)
}

// deletedOf is MakeDeltaMergeData's deleted set (awset-delta_test.go:93-102):
// tombstones whose key was not re-added with another or a newer dot.
func deletedOf(s docState) map[string]crdt.Dot {
	out := map[string]crdt.Dot{}
	for k, x := range s.Deleted {
		if m, ok := s.Entries[k]; ok && (m.Actor != x.Actor || m.Counter > x.Counter) {
			continue
		}
		out[k] = x
	}
	return out
}

// panic-free HasDot / Counter for foldWidth (a panicking batch never gets here)
func hasDotOf(vv crdt.VersionVector, d crdt.Dot) bool {
	return int(d.Actor) < len(vv) && vv[d.Actor] >= d.Counter
}

func counterOf(vv crdt.VersionVector, a crdt.Actor) uint {
	if int(a) < len(vv) {
		return vv[a]
	}
	return 0
}

func distinct(states []*crdt.AWSet) error {
	seen := make(map[*crdt.AWSet]struct{}, len(states))
	for _, s := range states {
		if _, ok := seen[s]; ok {
			return fmt.Errorf("a state appears twice as a destination of one batch")
		}
		seen[s] = struct{}{}
	}
	return nil
}

// ---------------------------------------------------------------- ragged clocks

// docState is one state of a document: the destination, or one of its
// ordered sources (Deleted: AWSetDelta.Deleted, nil for an AWSet).
type docState struct {
	Actor         crdt.Actor
	VersionVector crdt.VersionVector
	Entries       map[string]crdt.Dot
	Deleted       map[string]crdt.Dot
}

func stateOf(s *crdt.AWSet, deleted map[string]crdt.Dot) docState {
	return docState{s.Actor, s.VersionVector, s.Entries, deleted}
}

type goPanic struct{}

// checks evaluates HasDot / Counter as Go does on the unpadded vectors
// (crdt-misc.go:28-41) and notes where the zero-padded width R answers
// differently (a counter-0 dot at len(vv) < actor < R).
type checks struct {
	R          int
	padDiffers bool
}

func (c *checks) has(vv crdt.VersionVector, d crdt.Dot) bool {
	if len(vv) < int(d.Actor) {
		if int(d.Actor) < c.R && d.Counter == 0 {
			c.padDiffers = true
		}
		return false
	}
	if int(d.Actor) == len(vv) {
		panic(goPanic{})
	}
	return vv[d.Actor] >= d.Counter
}

func (c *checks) counter(vv crdt.VersionVector, a crdt.Actor) uint {
	if len(vv) < int(a) {
		return 0
	}
	if int(a) == len(vv) {
		panic(goPanic{})
	}
	return vv[a]
}

// replayChecks replays doc[0].Merge(doc[j]) for j = 1.. in order on copies of
// the maps, with the reference's rules (awset.go:107-161; for delta,
// awset-delta_test.go:51-166), only to learn whether Go panics (1) or the
// padded layout would differ (2). The merged entries come from the GPU.
func replayChecks(delta bool, doc []docState, R int) (res int) {
	c := checks{R: R}
	defer func() {
		if r := recover(); r != nil {
			if _, ok := r.(goPanic); !ok {
				panic(r)
			}
			res = 1
		}
	}()
	V := append(crdt.VersionVector(nil), doc[0].VersionVector...)
	E := make(map[string]crdt.Dot, len(doc[0].Entries))
	for k, d := range doc[0].Entries {
		E[k] = d
	}
	for _, s := range doc[1:] {
		full := !delta || c.counter(V, s.Actor) == 0 // awset-delta_test.go:53
		changed, deleted := s.Entries, map[string]crdt.Dot(nil)
		if !full { // MakeDeltaMergeData, awset-delta_test.go:79-105
			changed = map[string]crdt.Dot{}
			for k, d := range s.Entries {
				if !c.has(V, d) {
					changed[k] = d
				}
			}
			deleted = deletedOf(s)
			if len(changed) == 0 && len(deleted) == 0 {
				continue // :60 -- not even the VV merge
			}
		}
		for k, sd := range changed { // phase 1: awset.go:122-143, awset-delta_test.go:126-147
			if _, ok := E[k]; ok || !c.has(V, sd) {
				E[k] = sd
			}
		}
		if full { // phase 2: awset.go:145-159
			for k, d := range E {
				if _, ok := s.Entries[k]; !ok && c.has(s.VersionVector, d) {
					delete(E, k)
				}
			}
		} else { // phase 2: awset-delta_test.go:149-164
			for k, x := range deleted {
				if _, ok := E[k]; ok && !c.has(V, x) {
					delete(E, k)
				}
			}
		}
		V.Merge(s.VersionVector)
	}
	if c.padDiffers {
		return 2
	}
	return 0
}

// raggedChecks picks the batch's padded width R (>= every vector's length,
// clear of the actors of documents with a shorter vector: the kernels flag
// actor == R) and replays those documents. Equal-length documents need no
// host work: the kernels flag actor == R exactly where Go panics.
func raggedChecks(delta bool, docs [][]docState) (int, error) {
	R := 1
	for _, doc := range docs {
		for _, s := range doc {
			R = max(R, len(s.VersionVector))
		}
	}
	short := func(doc []docState, w int) bool {
		for _, s := range doc {
			if len(s.VersionVector) < w {
				return true
			}
		}
		return false
	}
	hasActor := func(doc []docState, w int) bool {
		for j, s := range doc {
			if j > 0 && delta && int(s.Actor) == w {
				return true
			}
			for _, m := range []map[string]crdt.Dot{s.Entries, s.Deleted} {
				for _, d := range m {
					if int(d.Actor) == w {
						return true
					}
				}
			}
		}
		return false
	}
	w := R
	for ; w <= C.CRDT_MAX_R; w++ {
		clash := false
		for _, doc := range docs {
			if short(doc, w) && hasActor(doc, w) {
				clash = true
				break
			}
		}
		if !clash {
			break
		}
	}
	if w > C.CRDT_MAX_R {
		return 0, fmt.Errorf("no padded width <= %d clear of the actors", C.CRDT_MAX_R)
	}
	for _, doc := range docs {
		if !short(doc, w) {
			continue
		}
		switch replayChecks(delta, doc, w) {
		case 1:
			return 0, &Error{"raggedChecks", int(C.CRDT_E_ACTOR_RANGE)} // Go panics here
		case 2:
			return 0, fmt.Errorf("counter-0 dot beyond a shorter version vector (not representable padded)")
		}
	}
	return w, nil
}
