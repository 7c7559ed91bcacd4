//go:build cgo && honu_hip

// Package object: the gfx950 batch codec behind Honu's pkg/store/object API.
//
// STATUS: UNVERIFIED. Neither the build container nor the GPU box of this
// repository has a Go toolchain (profiles/r01_gpu_box_toolchains.txt), so this
// file has never been compiled. It is the cgo binding a maintainer vendors
// into rotationalio/honu's pkg/store/object (INTEGRATION.md), kept behind the
// `honu_hip` build tag so the pure-Go Marshal / Metadata / Data stay the
// default (the reference builds with CGO_ENABLED=0, Dockerfile:24). The C ABI
// it calls (include/honu_codec.h) is exercised on the GPU from plain C by
// honu_amd/c_abi_demo.c, which runs this file's MarshalBatch / DecodeBatch
// call sequence (tests/test_c_abi.py), and from Python by the test suite.
//
// Reference functions replaced, one batch per call instead of one record:
//
//	object.Marshal            object.go:24-45  -> (*Codec).MarshalBatch
//	(Object).Metadata / Data  object.go:66-99  -> (*Codec).DecodeBatch
//	sort.Sort(keys.Keys)      keys/keys.go:126-130 -> (*Codec).SortKeys
//	object version ranges     keys/keys.go:73-92   -> (*Codec).KeyObjects
//	Cursor.Seek, Has, Exists  iterator/cursor.go:44-55, collection.go:47-65 -> (*Codec).SeekKeys, Has, Exists
//	pid.Next, Tombstone       lamport/pid.go:10-15, metadata/collection.go:56-63 -> (*Codec).NextVersions
//	lamport.Compare, two replicas  lamport/scalar.go:15-78, keys/keys.go:35-36 -> (*Codec).CompareKeys
//	Drop "to free up space"   store.go:314-322, 399-404 -> (*Codec).ReclaimRecords
//	tx.Bucket(collectionID)   store.go:236-240, tx.go:112-120 -> (*Codec).RouteKeys
package object

/*
#cgo CFLAGS: -I${SRCDIR}/internal/hip
#cgo LDFLAGS: -L${SRCDIR}/internal/hip -lhonu_codec -Wl,-rpath,${SRCDIR}/internal/hip
#include <stdlib.h>
#include "honu_codec.h"
*/
import "C"

import (
	"encoding/binary"
	"errors"
	"fmt"
	"io"
	"net"
	"time"
	"unsafe"

	"go.rtnl.ai/honu/pkg/region"
	"go.rtnl.ai/honu/pkg/store/keys"
	"go.rtnl.ai/honu/pkg/store/lamport"
	"go.rtnl.ai/honu/pkg/store/lani"
	"go.rtnl.ai/honu/pkg/store/metadata"
	"go.rtnl.ai/ulid"
)

var ErrGoPanic = errors.New("object: input on which the pure-Go codec panics")
var ErrInput = errors.New("object: a row's span or list lies outside its arena")
var ErrCapacity = errors.New("object: GPU output arena or table too small")

var statusErr = map[C.int32_t]error{
	C.HONU_ERR_BAD_VERSION:    ErrBadVersion,
	C.HONU_ERR_MALFORMED:      ErrMalformed,
	C.HONU_ERR_EOF:            io.EOF,
	C.HONU_ERR_UNEXPECTED_EOF: io.ErrUnexpectedEOF,
	C.HONU_ERR_NO_LENGTH:      lani.ErrNoLength,
	C.HONU_ERR_PARSE_BOOLEAN:  lani.ErrParseBoolean,
	C.HONU_ERR_PARSE_VARINT:   lani.ErrParseVarInt,
	C.HONU_ERR_PANIC:          ErrGoPanic,
	C.HONU_ERR_INPUT:          ErrInput,
	C.HONU_ERR_CAPACITY:       ErrCapacity,
}

// recordErr maps a per-record status to an error; an unknown code is an
// error too, so no failed record can come back as (nil, nil).
func recordErr(st C.int32_t) error {
	if st == C.HONU_OK {
		return nil
	}
	if err, ok := statusErr[st]; ok {
		return err
	}
	return fmt.Errorf("object: unknown codec status %d", int32(st))
}

// call checks a call-level status (HONU_E_ARG, HONU_E_WORKSPACE, HONU_E_HIP, ...).
func call(what string, st C.int32_t) error {
	if st == C.HONU_OK {
		return nil
	}
	return fmt.Errorf("%s: %s (%s)", what, C.GoString(C.honu_status_string(st)),
		C.GoString(C.honu_last_error()))
}

// Codec owns one device context. Buffers handed to C live in C memory
// (pinned host / device), never in the Go heap, so asynchronous GPU work
// obeys the cgo pointer-passing rules.
type Codec struct {
	ctx    *C.honu_ctx
	stream unsafe.Pointer // nil: the null stream
	// ACL table entries / regions per record of the last decoded batch: the
	// first guess for the next batch's table sizes (DecodeBatch). With the
	// ACL lists returned in place (the default) only lists holding a nil
	// entry take table entries.
	aclPerRecord, regPerRecord uint64
}

func NewCodec(device int, maxRecords uint64) (*Codec, error) {
	if v := C.honu_abi_version(); v != C.HONU_ABI_VERSION {
		return nil, fmt.Errorf("object: libhonu_codec ABI %d, this binding %d", v, C.HONU_ABI_VERSION)
	}
	var st C.int32_t
	ctx := C.honu_ctx_create(C.int(device), C.uint64_t(maxRecords), &st)
	if ctx == nil {
		return nil, errors.New(C.GoString(C.honu_status_string(st)))
	}
	return &Codec{ctx: ctx, aclPerRecord: 1, regPerRecord: 8}, nil
}

func (c *Codec) Close() { C.honu_ctx_destroy(c.ctx) }

// Param / SetParam: the context's launch parameters (honu_ctx_set_param,
// honu_ctx_get_param). "speculate" 0 turns the single-launch decode's
// speculation off for a context that mostly sees malformed records; without
// it the context backs off by itself for 16 calls after a recovery
// ("speculate_backoff" reads the calls left, "recoveries" counts them).
// "acl_inplace" 0 returns every ACL list in the table (unflatten reads both).
func (c *Codec) SetParam(name string, v int64) error {
	cs := C.CString(name)
	defer C.free(unsafe.Pointer(cs))
	if st := C.honu_ctx_set_param(c.ctx, cs, C.int64_t(v)); st != 0 {
		return errors.New(C.GoString(C.honu_last_error()))
	}
	return nil
}

func (c *Codec) Param(name string) (int64, error) {
	cs := C.CString(name)
	defer C.free(unsafe.Pointer(cs))
	var v C.int64_t
	if st := C.honu_ctx_get_param(c.ctx, cs, &v); st != 0 {
		return 0, errors.New(C.GoString(C.honu_last_error()))
	}
	return int64(v), nil
}

// hostBuf / devBuf: pinned host and device allocations owned by C.
type hostBuf struct {
	p unsafe.Pointer
	n uintptr
}
type devBuf struct {
	p unsafe.Pointer
	n uintptr
}

func pinned(n uintptr) hostBuf { return hostBuf{C.honu_host_alloc(C.uint64_t(n + 16)), n} }
func device(n uintptr) devBuf  { return devBuf{C.honu_device_alloc(C.uint64_t(n + 16)), n} }
func (h hostBuf) bytes() []byte { return unsafe.Slice((*byte)(h.p), h.n) }
func (h hostBuf) free()         { C.honu_host_free(h.p) }
func (d devBuf) free()          { C.honu_device_free(d.p) }

// batch: one flattened batch in pinned memory (the encode input of
// include/honu_codec.h: rows, var arena, ACL table, region table, CSR
// payload arena).
type batch struct {
	rows, vars, acls, regs, pay, payOff hostBuf
	n, nacl, nreg                       uint64
}

type devBatch struct{ rows, vars, acls, regs, pay, payOff devBuf }

func (b *batch) free() {
	for _, h := range []hostBuf{b.rows, b.vars, b.acls, b.regs, b.pay, b.payOff} {
		h.free()
	}
}

func (d *devBatch) free() {
	for _, x := range []devBuf{d.rows, d.vars, d.acls, d.regs, d.pay, d.payOff} {
		x.free()
	}
}

func (b *batch) upload(stream unsafe.Pointer) (*devBatch, error) {
	d := &devBatch{}
	for _, x := range []struct {
		h hostBuf
		d *devBuf
	}{{b.rows, &d.rows}, {b.vars, &d.vars}, {b.acls, &d.acls}, {b.regs, &d.regs}, {b.pay, &d.pay},
		{b.payOff, &d.payOff}} {
		*x.d = device(x.h.n)
		if x.d.p == nil {
			d.free()
			return nil, errors.New("object: device allocation failed")
		}
		if err := call("upload", C.honu_memcpy_h2d(x.d.p, x.h.p, C.uint64_t(x.h.n), stream)); err != nil {
			d.free()
			return nil, err
		}
	}
	return d, nil
}

func cULID(u ulid.ULID) (o [16]C.uint8_t) {
	for k := range o {
		o[k] = C.uint8_t(u[k])
	}
	return o
}

// nanos: lani.EncodeTime (lani/encode.go:201-206): 0 for the zero time.
func nanos(t time.Time) C.int64_t {
	if t.IsZero() {
		return 0
	}
	return C.int64_t(t.UnixNano())
}

// flatten writes one honu_meta row per *metadata.Metadata (presence bits from
// the nil pointers, ULIDs inline, strings and byte slices appended to the var
// arena as {off, len}, ACL entries and regions appended to their tables,
// times as UnixNano or 0), and the payloads as a CSR arena; mirrors
// honu_amd/metadata.py:pack_batch. A nil *Metadata leaves an all-zero row
// (no HONU_HAS_META): the encoder reports HONU_ERR_PANIC, where Marshal(nil,
// ...) panics (metadata.go:66).
func flatten(metas []*metadata.Metadata, datas [][]byte) *batch {
	n := uint64(len(metas))
	var nvar, nacl, nreg, npay uint64
	for i, m := range metas {
		npay += uint64(len(datas[i]))
		if m == nil {
			continue
		}
		nvar += uint64(len(m.MIME))
		if m.Schema != nil {
			nvar += uint64(len(m.Schema.Name))
		}
		if p := m.Publisher; p != nil {
			nvar += uint64(len(p.IPAddress) + len(p.UserAgent))
		}
		if e := m.Encryption; e != nil {
			nvar += uint64(len(e.PublicKeyID) + len(e.EncryptionKey) + len(e.HMACSecret) + len(e.Signature))
		}
		nacl += uint64(len(m.ACL))
		nreg += uint64(len(m.WriteRegions))
	}
	b := &batch{n: n, nacl: nacl, nreg: nreg,
		rows: pinned(uintptr(n) * uintptr(C.sizeof_honu_meta)), vars: pinned(uintptr(nvar)),
		acls: pinned(uintptr(nacl) * uintptr(C.sizeof_honu_acl)), regs: pinned(4 * uintptr(nreg)),
		pay: pinned(uintptr(npay)), payOff: pinned(8 * uintptr(n+1))}
	rows := unsafe.Slice((*C.honu_meta)(b.rows.p), n)
	vars, pay := b.vars.bytes(), b.pay.bytes()
	acls := unsafe.Slice((*C.honu_acl)(b.acls.p), nacl)
	regs := unsafe.Slice((*uint32)(b.regs.p), nreg)
	payOff := unsafe.Slice((*uint64)(b.payOff.p), n+1)
	var v, a, g, p uint64
	span := func(s []byte) C.honu_span {
		if len(s) == 0 { // nil and empty encode alike (lani/encode.go Encode)
			return C.honu_span{}
		}
		o := v
		v += uint64(copy(vars[v:], s))
		return C.honu_span{off: C.uint64_t(o), len: C.uint64_t(len(s))}
	}
	for i, m := range metas {
		payOff[i] = p
		p += uint64(copy(pay[p:], datas[i]))
		r := &rows[i]
		*r = C.honu_meta{}
		if m == nil {
			continue
		}
		pr := uint32(C.HONU_HAS_META)
		r.object_id, r.collection_id = cULID(m.ObjectID), cULID(m.CollectionID)
		if ver := m.Version; ver != nil {
			pr |= C.HONU_HAS_VERSION
			r.pid, r.vid, r.region = C.uint32_t(ver.Scalar.PID), C.uint64_t(ver.Scalar.VID), C.uint32_t(ver.Region)
			if ver.Parent != nil {
				pr |= C.HONU_HAS_PARENT
				r.parent_pid, r.parent_vid = C.uint32_t(ver.Parent.PID), C.uint64_t(ver.Parent.VID)
			}
			if ver.Tombstone {
				r.tombstone = 1
			}
			r.version_created = nanos(ver.Created)
		}
		if s := m.Schema; s != nil {
			pr |= C.HONU_HAS_SCHEMA
			r.schema_name = span([]byte(s.Name))
			r.schema_major, r.schema_minor, r.schema_patch = C.uint32_t(s.Major), C.uint32_t(s.Minor), C.uint32_t(s.Patch)
		}
		r.mime = span([]byte(m.MIME))
		r.owner, r.group = cULID(m.Owner), cULID(m.Group)
		r.permissions = C.uint8_t(m.Permissions)
		if len(m.ACL) > 0 {
			r.acl_off, r.acl_count = C.uint64_t(a), C.uint64_t(len(m.ACL))
			nb := uint64(0) // the list's encoded length, carried (HONU_ACL_SIZED): the size pass reads no entry
			for _, e := range m.ACL {
				acls[a] = C.honu_acl{}
				nb++ // a nil entry encodes as one 0x00 flag byte
				if e != nil {
					acls[a].client_id, acls[a].permissions, acls[a].present = cULID(e.ClientID), C.uint8_t(e.Permissions), 1
					nb += 17 // 01 | ClientID | Permissions (acls.go:26-39)
				}
				a++
			}
			r.acl_bytes = C.uint64_t(nb)
			pr |= C.HONU_ACL_SIZED
		}
		if len(m.WriteRegions) > 0 {
			r.regions_off, r.regions_count = C.uint64_t(g), C.uint64_t(len(m.WriteRegions))
			for _, x := range m.WriteRegions {
				regs[g] = uint32(x)
				g++
			}
		}
		if pub := m.Publisher; pub != nil {
			pr |= C.HONU_HAS_PUBLISHER
			r.publisher_id, r.client_id = cULID(pub.PublisherID), cULID(pub.ClientID)
			r.ip_address, r.user_agent = span(pub.IPAddress), span([]byte(pub.UserAgent))
		}
		if e := m.Encryption; e != nil {
			pr |= C.HONU_HAS_ENCRYPTION
			r.public_key_id, r.encryption_key = span([]byte(e.PublicKeyID)), span(e.EncryptionKey)
			r.hmac_secret, r.signature = span(e.HMACSecret), span(e.Signature)
			r.sealing_alg, r.encryption_alg = C.uint8_t(e.SealingAlgorithm), C.uint8_t(e.EncryptionAlgorithm)
			r.signature_alg = C.uint8_t(e.SignatureAlgorithm)
		}
		if cmp := m.Compression; cmp != nil {
			pr |= C.HONU_HAS_COMPRESSION
			r.compression_alg, r.compression_level = C.uint8_t(cmp.Algorithm), C.int64_t(cmp.Level)
		}
		r.flags = C.uint8_t(m.Flags)
		r.created, r.modified = nanos(m.Created), nanos(m.Modified)
		r.present = C.uint32_t(pr)
	}
	payOff[n] = p
	return b
}

// MarshalBatch is object.Marshal for many records in one GPU pass.
func (c *Codec) MarshalBatch(metas []*metadata.Metadata, datas [][]byte) ([]Object, []error, error) {
	n := len(metas)
	// 1. flatten into pinned C memory, 2. host -> device
	b := flatten(metas, datas)
	defer b.free()
	d, err := b.upload(c.stream)
	if err != nil {
		return nil, nil, err
	}
	defer d.free()
	// 3. sizes + exclusive scan -> output offsets; read the total back
	outOff, status, hOff := device(8*uintptr(n+1)), device(4*uintptr(n)), pinned(8*uintptr(n+1))
	defer outOff.free()
	defer status.free()
	defer hOff.free()
	if err := call("honu_encode_sizes", C.honu_encode_sizes(c.ctx, (*C.honu_meta)(d.rows.p),
		C.uint64_t(b.vars.n), (*C.honu_acl)(d.acls.p), C.uint64_t(b.nacl), (*C.uint32_t)(d.regs.p),
		C.uint64_t(b.nreg), (*C.uint64_t)(d.payOff.p), C.uint64_t(n), (*C.uint64_t)(outOff.p),
		(*C.int32_t)(status.p), c.stream)); err != nil {
		return nil, nil, err
	}
	// HONU_E_WORKSPACE here (n > the context's maxRecords) would leave outOff
	// unwritten: nothing below may read it then
	if err := call("honu_exclusive_scan", C.honu_exclusive_scan(c.ctx, (*C.uint64_t)(outOff.p),
		C.uint64_t(n), (*C.uint64_t)(outOff.p), c.stream)); err != nil {
		return nil, nil, err
	}
	if err := call("d2h", C.honu_memcpy_d2h(hOff.p, outOff.p, C.uint64_t(hOff.n), c.stream)); err != nil {
		return nil, nil, err
	}
	if err := call("sync", C.honu_stream_sync(c.stream)); err != nil {
		return nil, nil, err
	}
	offs := unsafe.Slice((*uint64)(hOff.p), n+1)
	// 4. encode into a device arena, copy the records back
	out := device(uintptr(offs[n]))
	defer out.free()
	if err := call("honu_encode", C.honu_encode(c.ctx, (*C.honu_meta)(d.rows.p),
		(*C.uint8_t)(d.vars.p), C.uint64_t(b.vars.n), (*C.honu_acl)(d.acls.p), C.uint64_t(b.nacl),
		(*C.uint32_t)(d.regs.p), C.uint64_t(b.nreg), (*C.uint8_t)(d.pay.p), (*C.uint64_t)(d.payOff.p),
		C.uint64_t(n), (*C.uint8_t)(out.p), C.uint64_t(out.n), (*C.uint64_t)(outOff.p),
		(*C.int32_t)(status.p), c.stream)); err != nil {
		return nil, nil, err
	}
	hOut, hSt := pinned(out.n), pinned(4*uintptr(n))
	defer hOut.free()
	defer hSt.free()
	for _, st := range []C.int32_t{
		C.honu_memcpy_d2h(hOut.p, out.p, C.uint64_t(out.n), c.stream),
		C.honu_memcpy_d2h(hSt.p, status.p, C.uint64_t(hSt.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("download", st); err != nil {
			return nil, nil, err
		}
	}
	objs, errs := make([]Object, n), make([]error, n)
	all, st := hOut.bytes(), unsafe.Slice((*int32)(hSt.p), n)
	for i := range objs {
		if errs[i] = recordErr(C.int32_t(st[i])); errs[i] != nil {
			continue
		}
		objs[i] = append(Object(nil), all[offs[i]:offs[i+1]]...) // caller-owned copy, like Marshal
	}
	return objs, errs, nil
}

// DecodeBatch is Object.Metadata + Object.Data for many records.
func (c *Codec) DecodeBatch(objs []Object) ([]*metadata.Metadata, [][]byte, []error, error) {
	n := len(objs)
	// 1. concatenate objs into a pinned arena with CSR offsets; upload
	var total uintptr
	for _, o := range objs {
		total += uintptr(len(o))
	}
	hArena, hOff := pinned(total), pinned(8*uintptr(n+1))
	defer hArena.free()
	defer hOff.free()
	arena, off := hArena.bytes(), unsafe.Slice((*uint64)(hOff.p), n+1)
	for i, o := range objs {
		off[i+1] = off[i] + uint64(copy(arena[off[i]:], o))
	}
	dArena, dOff := device(total), device(hOff.n)
	defer dArena.free()
	defer dOff.free()
	for _, st := range []C.int32_t{
		C.honu_memcpy_h2d(dArena.p, hArena.p, C.uint64_t(total), c.stream),
		C.honu_memcpy_h2d(dOff.p, hOff.p, C.uint64_t(hOff.n), c.stream),
	} {
		if err := call("upload", st); err != nil {
			return nil, nil, nil, err
		}
	}
	// 2. decode, zero copy: rows, record info, ACL / region tables. The tables
	//    are sized by ENTRY COUNTS, not record bytes (an entry takes >= 1 byte,
	//    so byte-sized tables would be 20 + 4 bytes per record byte: 24x the
	//    arena): start from the codec's running estimate, and when the batch
	//    needs more, the call's d_totals says exactly how many (records past a
	//    cap get HONU_ERR_CAPACITY and nothing else changes): re-allocate to the
	//    totals and decode again. An ACL list whose entries are all present
	//    comes back in place (HONU_ACL_INPLACE) and takes no table entry, and
	//    so does every region list (HONU_REGIONS_INPLACE): with the defaults
	//    only lists holding a nil ACL entry need the tables.
	//    honu_amd/c_abi_demo.c runs this flow in C.
	rows, info := device(uintptr(n)*uintptr(C.sizeof_honu_meta)), device(uintptr(n)*uintptr(C.sizeof_honu_record_info))
	tot, hTot := device(32), pinned(32)
	defer rows.free()
	defer info.free()
	defer tot.free()
	defer hTot.free()
	totals := unsafe.Slice((*uint64)(hTot.p), 4)
	aclCap, regCap := c.aclPerRecord*uint64(n)+64, c.regPerRecord*uint64(n)+64
	var acl, regs devBuf
	for try := 0; ; try++ {
		acl, regs = device(uintptr(aclCap)*uintptr(C.sizeof_honu_acl)), device(4*uintptr(regCap))
		if err := call("honu_decode_batch", C.honu_decode_batch(c.ctx, (*C.uint8_t)(dArena.p),
			(*C.uint64_t)(dOff.p), C.uint64_t(n), (*C.honu_meta)(rows.p), (*C.honu_record_info)(info.p),
			(*C.honu_acl)(acl.p), C.uint64_t(aclCap), (*C.uint32_t)(regs.p), C.uint64_t(regCap), nil, 0,
			(*C.uint64_t)(tot.p), c.stream)); err != nil {
			acl.free()
			regs.free()
			return nil, nil, nil, err // e.g. HONU_E_WORKSPACE: n > maxRecords, nothing was decoded
		}
		err := call("totals", C.honu_memcpy_d2h(hTot.p, tot.p, 24, c.stream))
		if err == nil {
			err = call("sync", C.honu_stream_sync(c.stream))
		}
		if err != nil {
			acl.free()
			regs.free()
			return nil, nil, nil, err
		}
		if totals[0] <= aclCap && totals[1] <= regCap {
			break
		}
		acl.free()
		regs.free()
		if try == 1 { // the totals of one batch do not change between calls
			return nil, nil, nil, fmt.Errorf("%w: ACL %d / regions %d", ErrCapacity, totals[0], totals[1])
		}
		aclCap, regCap = totals[0], totals[1]
	}
	defer acl.free()
	defer regs.free()
	c.aclPerRecord, c.regPerRecord = (totals[0]+uint64(n)-1)/uint64(n), (totals[1]+uint64(n)-1)/uint64(n)
	// 3. download rows, info, tables (the arena is already here: hArena)
	hRows, hInfo := pinned(rows.n), pinned(info.n)
	hAcl, hReg := pinned(uintptr(totals[0])*uintptr(C.sizeof_honu_acl)), pinned(4*uintptr(totals[1]))
	defer hRows.free()
	defer hInfo.free()
	defer hAcl.free()
	defer hReg.free()
	for _, st := range []C.int32_t{
		C.honu_memcpy_d2h(hRows.p, rows.p, C.uint64_t(rows.n), c.stream),
		C.honu_memcpy_d2h(hInfo.p, info.p, C.uint64_t(info.n), c.stream),
		C.honu_memcpy_d2h(hAcl.p, acl.p, C.uint64_t(hAcl.n), c.stream),
		C.honu_memcpy_d2h(hReg.p, regs.p, C.uint64_t(hReg.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("download", st); err != nil {
			return nil, nil, nil, err
		}
	}
	rs := unsafe.Slice((*C.honu_meta)(hRows.p), n)
	is := unsafe.Slice((*C.honu_record_info)(hInfo.p), n)
	as := unsafe.Slice((*C.honu_acl)(hAcl.p), totals[0])
	gs := unsafe.Slice((*uint32)(hReg.p), totals[1])
	metas, datas, errs := make([]*metadata.Metadata, n), make([][]byte, n), make([]error, n)
	for i := range objs {
		if errs[i] = recordErr(is[i].meta_status); errs[i] == nil { // else Metadata() returns nil, err
			metas[i] = unflatten(&rs[i], arena, as, gs)
		}
		if is[i].data_status == 0 && is[i].data_len > 0 { // Data(): a subslice of objs[i], as in Go
			b := uint64(is[i].data_off) - off[i]
			datas[i] = objs[i][b : b+uint64(is[i].data_len)]
		}
	}
	return metas, datas, errs, nil
}

// unflatten is the Go decoder's own construction from one decoded row: spans
// index the concatenated arena and are copied out (lani Decode copies frames,
// decode.go:50-51), a zero-length frame is nil (decode.go:37-39), ACL count 0
// is a nil slice (metadata.go:254), regions are always a non-nil slice
// (region.go:160), time 0 is time.Time{} (decode.go:224-237). An ACL list
// returned in place (HONU_ACL_INPLACE) is read from the arena: entry k is the
// 18 bytes 01 | ClientID | Permissions at acl_off + 18 k (acls.go:26-51);
// otherwise from the ACL table, where present == 0 is a nil entry. A region
// list returned in place (HONU_REGIONS_INPLACE) is read from the arena too.
func unflatten(r *C.honu_meta, arena []byte, acl []C.honu_acl, regs []uint32) *metadata.Metadata {
	frame := func(s C.honu_span) []byte {
		if s.len == 0 {
			return nil
		}
		return append([]byte(nil), arena[s.off:s.off+s.len]...)
	}
	ulidOf := func(b [16]C.uint8_t) (u ulid.ULID) {
		for k := range u {
			u[k] = byte(b[k])
		}
		return u
	}
	when := func(ns C.int64_t) time.Time {
		if ns == 0 {
			return time.Time{}
		}
		return time.Unix(0, int64(ns)).In(time.UTC)
	}
	p := uint32(r.present)
	if p&C.HONU_HAS_META == 0 {
		return &metadata.Metadata{} // nil-flag 0x00: a zero Metadata, no error (object.go:76-82)
	}
	m := &metadata.Metadata{
		ObjectID: ulidOf(r.object_id), CollectionID: ulidOf(r.collection_id),
		MIME: string(frame(r.mime)), Owner: ulidOf(r.owner), Group: ulidOf(r.group),
		Permissions: uint8(r.permissions), Flags: uint8(r.flags),
		Created: when(r.created), Modified: when(r.modified),
		WriteRegions: make(region.Regions, r.regions_count),
	}
	if p&C.HONU_HAS_VERSION != 0 {
		m.Version = &metadata.Version{
			Scalar:    lamport.Scalar{PID: uint32(r.pid), VID: uint64(r.vid)},
			Region:    region.Region(r.region),
			Tombstone: r.tombstone != 0,
			Created:   when(r.version_created),
		}
		if p&C.HONU_HAS_PARENT != 0 {
			m.Version.Parent = &lamport.Scalar{PID: uint32(r.parent_pid), VID: uint64(r.parent_vid)}
		}
	}
	if p&C.HONU_HAS_SCHEMA != 0 {
		m.Schema = &metadata.SchemaVersion{Name: string(frame(r.schema_name)),
			Major: uint32(r.schema_major), Minor: uint32(r.schema_minor), Patch: uint32(r.schema_patch)}
	}
	if r.acl_count > 0 {
		m.ACL = make([]*metadata.AccessControl, r.acl_count)
		if p&C.HONU_ACL_INPLACE != 0 {
			for k := range m.ACL {
				e := arena[uint64(r.acl_off)+18*uint64(k):][:18]
				var u ulid.ULID
				copy(u[:], e[1:17])
				m.ACL[k] = &metadata.AccessControl{ClientID: u, Permissions: e[17]}
			}
		} else {
			for k := range m.ACL {
				e := &acl[uint64(r.acl_off)+uint64(k)]
				if e.present != 0 { // a nil entry stays nil (acls.go:41-51)
					m.ACL[k] = &metadata.AccessControl{ClientID: ulidOf(e.client_id), Permissions: uint8(e.permissions)}
				}
			}
		}
	}
	if p&C.HONU_REGIONS_INPLACE != 0 {
		// in place: the list's uvarints in the arena, read as Regions.Decode
		// reads them (region.go:154-169 -> lani DecodeUint32: at most 5 bytes,
		// truncated to uint32, decode.go:127-146); the GPU decode validated them
		q := uint64(r.regions_off)
		for k := range m.WriteRegions {
			v, w := binary.Uvarint(arena[q:min(q+5, uint64(len(arena)))])
			m.WriteRegions[k] = region.Region(uint32(v))
			q += uint64(w)
		}
	} else {
		for k := range m.WriteRegions {
			m.WriteRegions[k] = region.Region(regs[uint64(r.regions_off)+uint64(k)])
		}
	}
	if p&C.HONU_HAS_PUBLISHER != 0 {
		m.Publisher = &metadata.Publisher{PublisherID: ulidOf(r.publisher_id), ClientID: ulidOf(r.client_id),
			IPAddress: net.IP(frame(r.ip_address)), UserAgent: string(frame(r.user_agent))}
	}
	if p&C.HONU_HAS_ENCRYPTION != 0 {
		m.Encryption = &metadata.Encryption{PublicKeyID: string(frame(r.public_key_id)),
			EncryptionKey: frame(r.encryption_key), HMACSecret: frame(r.hmac_secret), Signature: frame(r.signature),
			SealingAlgorithm:    metadata.EncryptionAlgorithm(r.sealing_alg),
			EncryptionAlgorithm: metadata.EncryptionAlgorithm(r.encryption_alg),
			SignatureAlgorithm:  metadata.EncryptionAlgorithm(r.signature_alg)}
	}
	if p&C.HONU_HAS_COMPRESSION != 0 {
		m.Compression = &metadata.Compression{Algorithm: metadata.CompressionAlgorithm(r.compression_alg),
			Level: int64(r.compression_level)}
	}
	return m
}

// KeyOrder is the result of SortKeys: the order on the host, and the device
// buffers KeyObjects reads (the key column, the order, the valid count and
// the workspace both calls share). Free releases them.
//
// UNCOMPILED, like the rest of this file. The two calls are exercised on the
// GPU from Python (tests/test_gpu_sort.py), graph capture included.
type KeyOrder struct {
	Order []uint32 // record indices: [0, Valid) in bytes.Compare order of their keys, then the rest
	Valid uint64   // keys of the right size (the others sort last, in index order)

	n                                uint64
	keys, order, sorted, valid, work devBuf // sorted: the column in order, which SeekKeys searches
	workBytes                uint64
}

func (o *KeyOrder) Free() {
	for _, d := range []devBuf{o.keys, o.order, o.sorted, o.valid, o.work} {
		d.free()
	}
}

// SortKeys is sort.Sort(keys.Keys) (keys/keys.go:126-130: Less is
// bytes.Compare < 0) on the GPU, made stable: equal keys keep their index
// order. It does not move ks; it returns the order. A key that is not 29
// bytes long takes no part (status HONU_ERR_MALFORMED) and sorts last.
func (c *Codec) SortKeys(ks [][]byte) (*KeyOrder, error) {
	n := uint64(len(ks))
	hKeys, hSt := pinned(uintptr(C.HONU_KEY_LEN*n)), pinned(uintptr(4*n))
	defer hKeys.free()
	defer hSt.free()
	col, st := hKeys.bytes(), unsafe.Slice((*C.int32_t)(hSt.p), n)
	for i, k := range ks {
		if len(k) == C.HONU_KEY_LEN {
			copy(col[C.HONU_KEY_LEN*i:], k)
			st[i] = C.HONU_OK
		} else {
			st[i] = C.HONU_ERR_MALFORMED
		}
	}
	o := &KeyOrder{n: n, workBytes: uint64(C.honu_sort_keys_workspace(C.uint64_t(n)))}
	o.keys, o.order, o.valid = device(hKeys.n), device(uintptr(4*n)), device(8)
	o.sorted = device(hKeys.n)
	o.work = device(uintptr(o.workBytes)) // hipMalloc: 256-byte aligned
	dSt := device(hSt.n)
	defer dSt.free()
	hOrder, hValid := pinned(uintptr(4*n)), pinned(8)
	defer hOrder.free()
	defer hValid.free()
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(o.keys.p, hKeys.p, C.uint64_t(hKeys.n), c.stream),
		C.honu_memcpy_h2d(dSt.p, hSt.p, C.uint64_t(hSt.n), c.stream),
		C.honu_sort_keys(c.ctx, (*C.uint8_t)(o.keys.p), (*C.int32_t)(dSt.p), C.uint64_t(n),
			(*C.uint32_t)(o.order.p), (*C.uint8_t)(o.sorted.p), (*C.uint64_t)(o.valid.p), o.work.p,
			C.uint64_t(o.workBytes), c.stream),
		C.honu_memcpy_d2h(hOrder.p, o.order.p, C.uint64_t(4*n), c.stream),
		C.honu_memcpy_d2h(hValid.p, o.valid.p, 8, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_sort_keys", s); err != nil {
			o.Free()
			return nil, err
		}
	}
	o.Order = append([]uint32(nil), unsafe.Slice((*uint32)(hOrder.p), n)...)
	o.Valid = *(*uint64)(hValid.p)
	return o, nil
}

// KeyObjects cuts a sorted order into objects: what a read of "the latest
// version ... or all versions related to the object" ranges over
// (keys.go:40-41), [ObjectPrefix, ObjectLimit) (keys.go:73-92). Object j has
// the versions o.Order[offsets[j]:offsets[j+1]], oldest first by
// lamport.Compare (lamport/scalar.go:50-78), and latest[j] is the index of its
// newest. Groups are by equality of the 17-byte prefix (ObjectLimit's
// limit[16]++ wraps for an ObjectID ending in 0xff; that is not reproduced).
func (c *Codec) KeyObjects(o *KeyOrder) (offsets []uint64, latest []uint32, err error) {
	n := o.n
	dOff, dLatest, dObjects := device(uintptr(8*(n+1))), device(uintptr(4*n)), device(8)
	defer dOff.free()
	defer dLatest.free()
	defer dObjects.free()
	hOff, hLatest, hObjects := pinned(uintptr(8*(n+1))), pinned(uintptr(4*n)), pinned(8)
	defer hOff.free()
	defer hLatest.free()
	defer hObjects.free()
	for _, s := range []C.int32_t{
		C.honu_key_objects(c.ctx, (*C.uint8_t)(o.keys.p), (*C.uint32_t)(o.order.p), (*C.uint64_t)(o.valid.p),
			C.uint64_t(n), (*C.uint64_t)(dOff.p), (*C.uint32_t)(dLatest.p), (*C.uint64_t)(dObjects.p),
			o.work.p, C.uint64_t(o.workBytes), c.stream),
		C.honu_memcpy_d2h(hObjects.p, dObjects.p, 8, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_objects", s); err != nil {
			return nil, nil, err
		}
	}
	objects := *(*uint64)(hObjects.p)
	for _, s := range []C.int32_t{ // only what was written: objects + 1 offsets, objects indices
		C.honu_memcpy_d2h(hOff.p, dOff.p, C.uint64_t(8*(objects+1)), c.stream),
		C.honu_memcpy_d2h(hLatest.p, dLatest.p, C.uint64_t(4*objects), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("download", s); err != nil {
			return nil, nil, err
		}
	}
	offsets = append([]uint64(nil), unsafe.Slice((*uint64)(hOff.p), objects+1)...)
	latest = append([]uint32(nil), unsafe.Slice((*uint32)(hLatest.p), objects)...)
	return offsets, latest, nil
}

// Seek is one row of SeekKeys: honu_seek (include/honu_codec.h).
//
// UNCOMPILED, like the rest of this file. honu_key_seek is exercised on the
// GPU from Python (tests/test_gpu_key_seek.py), graph capture included.
type Seek struct {
	Pos, End      uint32 // Cursor.Seek's position in the sorted order; [Pos, End) are the probe's keys
	First, Latest uint32 // o.Order[Pos], o.Order[End-1]: record indices (C.HONU_SEEK_NONE unless Found)
	Flags         uint32 // C.HONU_SEEK_*
}

func (s Seek) Found() bool { return s.Flags&C.HONU_SEEK_FOUND != 0 }

// SeekKeys is iterator.Cursor.Seek (iterator/cursor.go:44-55) for a batch of
// probes over a sorted order: for probe q, the first position whose key is >=
// probes[q] by bytes.Compare (o.Valid when there is none: Seek returns nil),
// and the position past the last key that has probes[q] as prefix. Every probe
// has the same length, 0..29: 29 a key, 17 an ObjectPrefix (keys.go:74-79), 16
// a bare id as Collection.Has passes it. info (the decode's record info rows on
// the device, or a zero devBuf) enables the two LIVE flags.
func (c *Codec) SeekKeys(o *KeyOrder, probes [][]byte, info devBuf) ([]Seek, error) {
	m := uint64(len(probes))
	if m == 0 {
		return nil, nil
	}
	plen := len(probes[0])
	if plen > C.HONU_KEY_LEN {
		return nil, fmt.Errorf("a probe is at most %d bytes", C.HONU_KEY_LEN)
	}
	hP, hOut := pinned(uintptr(C.HONU_KEY_LEN*m)), pinned(uintptr(uint64(C.honu_sizeof_seek())*m))
	defer hP.free()
	defer hOut.free()
	col := hP.bytes()
	for q, p := range probes {
		if len(p) != plen {
			return nil, fmt.Errorf("probe %d: %d bytes, the batch's probes have %d", q, len(p), plen)
		}
		copy(col[C.HONU_KEY_LEN*q:], p) // the row's other bytes are not compared
	}
	dP, dOut := device(hP.n), device(hOut.n)
	defer dP.free()
	defer dOut.free()
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(dP.p, hP.p, C.uint64_t(hP.n), c.stream),
		C.honu_key_seek(c.ctx, (*C.uint8_t)(o.sorted.p), (*C.uint64_t)(o.valid.p), C.uint64_t(o.n),
			(*C.uint8_t)(dP.p), nil, C.uint32_t(plen), C.uint64_t(m), (*C.uint32_t)(o.order.p),
			(*C.honu_record_info)(info.p), (*C.honu_seek)(dOut.p), c.stream),
		C.honu_memcpy_d2h(hOut.p, dOut.p, C.uint64_t(hOut.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_key_seek", s); err != nil {
			return nil, err
		}
	}
	rows := unsafe.Slice((*C.honu_seek)(hOut.p), m)
	out := make([]Seek, m)
	for q, r := range rows {
		out[q] = Seek{uint32(r.pos), uint32(r.end), uint32(r.first), uint32(r.latest), uint32(r.flags)}
	}
	return out, nil
}

// MergeKeys is a batch of Puts into an ordered bucket (collections.Put,
// store.go:232, 395; collectionsBucket.Put, store.go:530; the bkt.Put(k, value)
// calls of iterator/cursor_test.go:235): the stable merge of a resident sorted
// order with a sorted batch, both from SortKeys or an earlier MergeKeys. The
// result is what SortKeys returns for the keys of a followed by the keys of b:
// b's record indices are its own plus a's count, equal keys stay one run with
// a's records before b's, and the run's last record, Seek.Latest, is the
// latest arrival, where bbolt's Put of a stored key replaces its value. a and
// b are not changed and stay the caller's to Free. The result takes SeekKeys,
// Has, Exists and a further MergeKeys; it holds no key column of its own, so
// KeyObjects is for an order that SortKeys made.
//
// UNCOMPILED, like the rest of this file. honu_key_merge is exercised on the
// GPU from Python (tests/test_gpu_key_merge.py), graph capture included.
func (c *Codec) MergeKeys(a, b *KeyOrder) (*KeyOrder, error) {
	n := a.n + b.n
	if n > 0xFFFFFFFF {
		return nil, fmt.Errorf("%d keys: an order indexes at most 2^32 - 1", n)
	}
	o := &KeyOrder{n: n}
	o.order, o.sorted, o.valid = device(uintptr(4*n)), device(uintptr(C.HONU_KEY_LEN*n)), device(8)
	hOrder, hValid := pinned(uintptr(4*n)), pinned(8)
	defer hOrder.free()
	defer hValid.free()
	for _, s := range []C.int32_t{
		C.honu_key_merge(c.ctx, (*C.uint8_t)(a.sorted.p), (*C.uint32_t)(a.order.p), (*C.uint64_t)(a.valid.p),
			C.uint64_t(a.n), (*C.uint8_t)(b.sorted.p), (*C.uint32_t)(b.order.p), (*C.uint64_t)(b.valid.p),
			C.uint64_t(b.n), C.uint32_t(a.n), (*C.uint8_t)(o.sorted.p), (*C.uint32_t)(o.order.p),
			(*C.uint64_t)(o.valid.p), c.stream),
		C.honu_memcpy_d2h(hOrder.p, o.order.p, C.uint64_t(4*n), c.stream),
		C.honu_memcpy_d2h(hValid.p, o.valid.p, 8, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_key_merge", s); err != nil {
			o.Free()
			return nil, err
		}
	}
	o.Order = append([]uint32(nil), unsafe.Slice((*uint32)(hOrder.p), n)...)
	o.Valid = *(*uint64)(hValid.p)
	return o, nil
}

// DeleteKeys is a batch of Deletes from an ordered bucket: the loop "Delete all
// collection versions" of Store.Drop (store.go:378-383: cursor.Seek(id[:]),
// then collections.Delete(key) while bytes.HasPrefix(key, id[:])) and the
// tx.DeleteBucket behind it (store.go:399-404). del is the SortKeys order of
// the keys to delete, of which only the first probeLen bytes count: 29 a key,
// 17 an ObjectPrefix, 16 a bare id, 0 everything; nil deletes by no list. With
// superseded every record that a later record of the same key replaced goes as
// well (bbolt's Put of a stored key replaces its value; MergeKeys keeps the
// run), so a key's Seek range is one row again. The loop in store.go deletes
// while it walks with cursor.Next(), which bbolt documents as able to skip
// keys; this does what the loop states, every key with the prefix. The result
// is an order like SortKeys': Valid counts the records that stay, and
// Order[Valid : Valid+removed] are the records that went, in key order, whose
// values the caller frees. o and del are not changed and stay the caller's to
// Free. The result takes SeekKeys, Has, Exists, MergeKeys and a further
// DeleteKeys.
//
// UNCOMPILED, like the rest of this file. honu_key_delete is exercised on the
// GPU from Python (tests/test_gpu_key_delete.py), graph capture included.
func (c *Codec) DeleteKeys(o, del *KeyOrder, probeLen int, superseded bool) (out *KeyOrder, removed uint64, err error) {
	n := o.n
	out = &KeyOrder{n: n}
	out.order, out.sorted, out.valid = device(uintptr(4*n)), device(uintptr(C.HONU_KEY_LEN*n)), device(8)
	workBytes := uint64(C.honu_key_delete_workspace(C.uint64_t(n)))
	work, dRemoved := device(uintptr(workBytes)), device(8)
	defer work.free()
	defer dRemoved.free()
	hOrder, hCounts := pinned(uintptr(4*n)), pinned(16)
	defer hOrder.free()
	defer hCounts.free()
	var dSorted *C.uint8_t
	var dValid *C.uint64_t
	var m C.uint64_t
	if del != nil && del.n > 0 {
		dSorted, dValid, m = (*C.uint8_t)(del.sorted.p), (*C.uint64_t)(del.valid.p), C.uint64_t(del.n)
	}
	var flags C.uint32_t
	if superseded {
		flags = C.HONU_DELETE_SUPERSEDED
	}
	for _, s := range []C.int32_t{
		C.honu_key_delete(c.ctx, (*C.uint8_t)(o.sorted.p), (*C.uint32_t)(o.order.p), (*C.uint64_t)(o.valid.p),
			C.uint64_t(n), dSorted, dValid, m, C.uint32_t(probeLen), flags, (*C.uint8_t)(out.sorted.p),
			(*C.uint32_t)(out.order.p), (*C.uint64_t)(out.valid.p), (*C.uint64_t)(dRemoved.p), work.p,
			C.uint64_t(workBytes), c.stream),
		C.honu_memcpy_d2h(hOrder.p, out.order.p, C.uint64_t(4*n), c.stream),
		C.honu_memcpy_d2h(hCounts.p, out.valid.p, 8, c.stream),
		C.honu_memcpy_d2h(unsafe.Add(hCounts.p, 8), dRemoved.p, 8, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_key_delete", s); err != nil {
			out.Free()
			return nil, 0, err
		}
	}
	out.Order = append([]uint32(nil), unsafe.Slice((*uint32)(hOrder.p), n)...)
	out.Valid = *(*uint64)(hCounts.p)
	return out, *(*uint64)(unsafe.Add(hCounts.p, 8)), nil
}

// ListRow is one row of ListKeys: honu_list_row (include/honu_codec.h).
type ListRow struct {
	Range  uint32 // which of the seeks it came from
	Pos    uint32 // position in the sorted order
	Record uint32 // o.Order[Pos]
	Flags  uint32 // C.HONU_LIST_ROW_*
}

func (r ListRow) Head() bool      { return r.Flags&C.HONU_LIST_ROW_HEAD != 0 }
func (r ListRow) Tombstone() bool { return r.Flags&C.HONU_LIST_ROW_TOMBSTONE != 0 }

// ListKeys is what follows the Seek on every read path, the walk with
// Cursor.Next() or Cursor.Prev() (iterator/cursor.go:57-89), for a batch of
// ranges: Collection.List (collection.go:32-35), Versions ("from the most
// recent version to the oldest", collection.go:106-110), Retrieve ("the latest
// version", collection.go:97-104) and the loop of store.go:379. seeks are
// SeekKeys' rows; for each, the rows a cursor over [Pos, End) visits, the
// ranges in order: forward from Pos, or with reverse from End-1 down; limit
// (not 0) stops each walk after that many rows, so reverse with limit 1 is the
// latest version of each range. With latest only the last row of every object
// (the keys that share an ObjectPrefix, keys.go:74-79) is visited. offsets[q]
// is where range q's rows start in rows and offsets[len(seeks)] their number.
// info (the decode's record info rows on the device, or a zero devBuf) sets
// Tombstone; tombstones are flagged here and filtered by FilterRows
// (collection.go:132-134); the record values of the rows are FetchObjects'. The first call counts, the
// second emits: the total is the one host round trip.
//
// UNCOMPILED, like the rest of this file. honu_key_list is exercised on the
// GPU from Python (tests/test_gpu_key_list.py), graph capture included.
func (c *Codec) ListKeys(o *KeyOrder, seeks []Seek, limit uint32, reverse, latest bool, info devBuf) (rows []ListRow, offsets []uint64, err error) {
	m := uint64(len(seeks))
	n := o.n
	seekSize, rowSize := uint64(C.honu_sizeof_seek()), uint64(C.honu_sizeof_list_row())
	hSeek, hOff := pinned(uintptr(seekSize*m)), pinned(uintptr(8*(m+1)))
	defer hSeek.free()
	defer hOff.free()
	in := unsafe.Slice((*C.honu_seek)(hSeek.p), m)
	for q, s := range seeks {
		in[q].pos, in[q].end, in[q].first = C.uint32_t(s.Pos), C.uint32_t(s.End), C.uint32_t(s.First)
		in[q].latest, in[q].flags = C.uint32_t(s.Latest), C.uint32_t(s.Flags)
	}
	dSeek, dOff, dTotal := device(hSeek.n), device(hOff.n), device(8)
	defer dSeek.free()
	defer dOff.free()
	defer dTotal.free()
	var flags C.uint32_t
	if reverse {
		flags |= C.HONU_LIST_REVERSE
	}
	var dObjOff, dLatest, dObjects, work devBuf
	if latest {
		if o.keys.p == nil { // MergeKeys and DeleteKeys return no key column in record order
			return nil, nil, fmt.Errorf("latest needs an order that SortKeys returned")
		}
		flags |= C.HONU_LIST_LATEST
		workBytes := uint64(C.honu_sort_keys_workspace(C.uint64_t(n)))
		dObjOff, dLatest, dObjects, work = device(uintptr(8*(n+1))), device(uintptr(4*n)), device(8), device(uintptr(workBytes))
		defer dObjOff.free()
		defer dLatest.free()
		defer dObjects.free()
		defer work.free()
		if err = call("honu_key_objects", C.honu_key_objects(c.ctx, (*C.uint8_t)(o.keys.p), (*C.uint32_t)(o.order.p),
			(*C.uint64_t)(o.valid.p), C.uint64_t(n), (*C.uint64_t)(dObjOff.p), (*C.uint32_t)(dLatest.p),
			(*C.uint64_t)(dObjects.p), work.p, C.uint64_t(workBytes), c.stream)); err != nil {
			return nil, nil, err
		}
	}
	list := func(dRows devBuf, cap uint64) C.int32_t {
		return C.honu_key_list(c.ctx, (*C.uint8_t)(o.sorted.p), (*C.uint32_t)(o.order.p), (*C.uint64_t)(o.valid.p),
			C.uint64_t(n), (*C.honu_seek)(dSeek.p), C.uint64_t(m), C.uint32_t(limit), flags,
			(*C.uint64_t)(dObjOff.p), (*C.uint64_t)(dObjects.p), (*C.honu_record_info)(info.p),
			(*C.uint64_t)(dOff.p), (*C.honu_list_row)(dRows.p), nil, C.uint64_t(cap), (*C.uint64_t)(dTotal.p), c.stream)
	}
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(dSeek.p, hSeek.p, C.uint64_t(hSeek.n), c.stream),
		list(devBuf{}, 0), // counts only
		C.honu_memcpy_d2h(hOff.p, dOff.p, C.uint64_t(hOff.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_list", s); err != nil {
			return nil, nil, err
		}
	}
	offsets = append([]uint64(nil), unsafe.Slice((*uint64)(hOff.p), m+1)...)
	total := offsets[m]
	if total == 0 {
		return nil, offsets, nil
	}
	hRows, dRows := pinned(uintptr(rowSize*total)), device(uintptr(rowSize*total))
	defer hRows.free()
	defer dRows.free()
	for _, s := range []C.int32_t{
		list(dRows, total),
		C.honu_memcpy_d2h(hRows.p, dRows.p, C.uint64_t(hRows.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_list", s); err != nil {
			return nil, nil, err
		}
	}
	rows = make([]ListRow, total)
	for g, r := range unsafe.Slice((*C.honu_list_row)(hRows.p), total) {
		rows[g] = ListRow{uint32(r._range), uint32(r.pos), uint32(r.record), uint32(r.flags)}
	}
	return rows, offsets, nil
}

// FetchObjects is Cursor.Object() (iterator/cursor.go:31-38: make + copy of
// the value under the cursor) for the rows of ListKeys: the step List, Versions
// and Retrieve (collection.go:32-35, 97-110) end in. rec, recOff (nrec + 1
// offsets) and recBytes are the records arena on the device; values[g] is the
// record rows[g] names, nil where its index or offsets are out of range
// (HONU_ERR_INPUT) and, with live, where the row is a tombstone (the object a
// listing does not return, collection.go:132-134; the row stays in place). The
// first call sizes (val_cap 0), the second copies: the byte total is the one
// host round trip. A caller that decodes on the device keeps dValues and
// dValOff there instead: they are the arena and offsets of honu_decode_batch.
//
// UNCOMPILED, like the rest of this file. honu_key_fetch is exercised on the
// GPU from Python (tests/test_gpu_key_fetch.py), graph capture included.
func (c *Codec) FetchObjects(rows []ListRow, rec, recOff devBuf, nrec, recBytes uint64, live bool) (values [][]byte, err error) {
	w := uint64(len(rows))
	if w == 0 {
		return nil, nil
	}
	rowSize := uint64(C.honu_sizeof_list_row())
	hRows, hOff, hStatus, hTotal := pinned(uintptr(rowSize*w)), pinned(uintptr(8*(w+1))), pinned(uintptr(4*w)), pinned(8)
	defer hRows.free()
	defer hOff.free()
	defer hStatus.free()
	defer hTotal.free()
	in := unsafe.Slice((*C.honu_list_row)(hRows.p), w)
	for g, r := range rows {
		in[g]._range, in[g].pos, in[g].record, in[g].flags = C.uint32_t(r.Range), C.uint32_t(r.Pos), C.uint32_t(r.Record), C.uint32_t(r.Flags)
	}
	*(*uint64)(hTotal.p) = w
	dRows, dTotal, dOff, dStatus, dNeed := device(hRows.n), device(8), device(hOff.n), device(hStatus.n), device(8)
	defer dRows.free()
	defer dTotal.free()
	defer dOff.free()
	defer dStatus.free()
	defer dNeed.free()
	var flags C.uint32_t
	if live {
		flags |= C.HONU_FETCH_LIVE
	}
	fetch := func(dValues devBuf, valCap uint64) C.int32_t {
		return C.honu_key_fetch(c.ctx, (*C.honu_list_row)(dRows.p), (*C.uint64_t)(dTotal.p), C.uint64_t(w),
			(*C.uint8_t)(rec.p), (*C.uint64_t)(recOff.p), C.uint64_t(nrec), C.uint64_t(recBytes), flags,
			(*C.uint64_t)(dOff.p), (*C.int32_t)(dStatus.p), (*C.uint8_t)(dValues.p), C.uint64_t(valCap),
			(*C.uint64_t)(dNeed.p), c.stream)
	}
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(dRows.p, hRows.p, C.uint64_t(hRows.n), c.stream),
		C.honu_memcpy_h2d(dTotal.p, hTotal.p, 8, c.stream),
		fetch(devBuf{}, 0), // sizes only
		C.honu_memcpy_d2h(hOff.p, dOff.p, C.uint64_t(hOff.n), c.stream),
		C.honu_memcpy_d2h(hStatus.p, dStatus.p, C.uint64_t(hStatus.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_fetch", s); err != nil {
			return nil, err
		}
	}
	off := unsafe.Slice((*uint64)(hOff.p), w+1)
	status := unsafe.Slice((*int32)(hStatus.p), w)
	values = make([][]byte, w)
	need := off[w]
	if need == 0 {
		return values, nil
	}
	hValues, dValues := pinned(uintptr(need)), device(uintptr(need))
	defer hValues.free()
	defer dValues.free()
	for _, s := range []C.int32_t{
		fetch(dValues, need),
		C.honu_memcpy_d2h(hValues.p, dValues.p, C.uint64_t(need), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_fetch", s); err != nil {
			return nil, err
		}
	}
	all := unsafe.Slice((*byte)(hValues.p), need)
	for g := range values {
		if status[g] == C.HONU_OK && !(live && rows[g].Tombstone()) {
			values[g] = append([]byte{}, all[off[g]:off[g+1]]...) // Object()'s make + copy
		}
	}
	return values, nil
}

// FilterRows is what a listing leaves out: an object deleted with a tombstone
// version "will not be returned in list queries or retrieval"
// (collection.go:132-134), and Retrieve of it is "not found"
// (collection.go:97-101). rows and offsets are ListKeys'; the rows that stay
// come back in order, with offsets[q] where range q's kept rows start,
// offsets[len(offsets)-1] their number and Head on the first kept row of each
// range, so they pass to FetchObjects as they are: an empty range is "not
// found". With tombstones a row whose Tombstone is set goes (the list was made
// with info): right for lists of latest versions. With deleted every row of an
// object whose latest version is a tombstone goes, wherever that version lies,
// and an older tombstone version of a live object stays (Versions "includes
// tombstone versions", collection.go:106-107); it needs info, the decode's
// record info rows on the device, and an order that SortKeys returned.
//
// UNCOMPILED, like the rest of this file. honu_key_filter is exercised on the
// GPU from Python (tests/test_gpu_key_filter.py), graph capture included.
func (c *Codec) FilterRows(o *KeyOrder, rows []ListRow, offsets []uint64, tombstones, deleted bool, info devBuf) (kept []ListRow, keptOffsets []uint64, err error) {
	w, m := uint64(len(rows)), uint64(len(offsets))-1
	n := o.n
	if w == 0 {
		return nil, make([]uint64, m+1), nil
	}
	rowSize := uint64(C.honu_sizeof_list_row())
	hRows, hOff, hTotal := pinned(uintptr(rowSize*w)), pinned(uintptr(8*(m+1))), pinned(8)
	defer hRows.free()
	defer hOff.free()
	defer hTotal.free()
	in := unsafe.Slice((*C.honu_list_row)(hRows.p), w)
	for g, r := range rows {
		in[g]._range, in[g].pos, in[g].record, in[g].flags = C.uint32_t(r.Range), C.uint32_t(r.Pos), C.uint32_t(r.Record), C.uint32_t(r.Flags)
	}
	copy(unsafe.Slice((*uint64)(hOff.p), m+1), offsets)
	*(*uint64)(hTotal.p) = w
	workBytes := uint64(C.honu_key_filter_workspace(C.uint64_t(w)))
	dRows, dOff, dTotal := device(hRows.n), device(hOff.n), device(8)
	dRowsOut, dOffOut, dTotalOut, work := device(hRows.n), device(hOff.n), device(8), device(uintptr(workBytes))
	for _, b := range []devBuf{dRows, dOff, dTotal, dRowsOut, dOffOut, dTotalOut, work} {
		defer b.free()
	}
	var flags C.uint32_t
	if tombstones {
		flags |= C.HONU_FILTER_TOMBSTONE
	}
	var dObjOff, dLatest, dObjects devBuf
	if deleted {
		if o.keys.p == nil || info.p == nil {
			return nil, nil, fmt.Errorf("deleted needs an order that SortKeys returned and the record info")
		}
		flags |= C.HONU_FILTER_DELETED
		sortBytes := uint64(C.honu_sort_keys_workspace(C.uint64_t(n)))
		sortWork := device(uintptr(sortBytes))
		dObjOff, dLatest, dObjects = device(uintptr(8*(n+1))), device(uintptr(4*n)), device(8)
		for _, b := range []devBuf{sortWork, dObjOff, dLatest, dObjects} {
			defer b.free()
		}
		if err = call("honu_key_objects", C.honu_key_objects(c.ctx, (*C.uint8_t)(o.keys.p), (*C.uint32_t)(o.order.p),
			(*C.uint64_t)(o.valid.p), C.uint64_t(n), (*C.uint64_t)(dObjOff.p), (*C.uint32_t)(dLatest.p),
			(*C.uint64_t)(dObjects.p), sortWork.p, C.uint64_t(sortBytes), c.stream)); err != nil {
			return nil, nil, err
		}
	}
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(dRows.p, hRows.p, C.uint64_t(hRows.n), c.stream),
		C.honu_memcpy_h2d(dOff.p, hOff.p, C.uint64_t(hOff.n), c.stream),
		C.honu_memcpy_h2d(dTotal.p, hTotal.p, 8, c.stream),
		C.honu_key_filter(c.ctx, (*C.honu_list_row)(dRows.p), nil, (*C.uint64_t)(dOff.p), C.uint64_t(m),
			(*C.uint64_t)(dTotal.p), C.uint64_t(w), flags, (*C.uint64_t)(o.valid.p), C.uint64_t(n),
			(*C.uint64_t)(dObjOff.p), (*C.uint32_t)(dLatest.p), (*C.uint64_t)(dObjects.p),
			(*C.honu_record_info)(info.p), (*C.honu_list_row)(dRowsOut.p), nil, (*C.uint64_t)(dOffOut.p),
			(*C.uint64_t)(dTotalOut.p), work.p, C.uint64_t(workBytes), c.stream),
		C.honu_memcpy_d2h(hRows.p, dRowsOut.p, C.uint64_t(hRows.n), c.stream),
		C.honu_memcpy_d2h(hOff.p, dOffOut.p, C.uint64_t(hOff.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_filter", s); err != nil {
			return nil, nil, err
		}
	}
	keptOffsets = append([]uint64(nil), unsafe.Slice((*uint64)(hOff.p), m+1)...)
	kept = make([]ListRow, keptOffsets[m])
	for g, r := range unsafe.Slice((*C.honu_list_row)(hRows.p), keptOffsets[m]) {
		kept[g] = ListRow{uint32(r._range), uint32(r.pos), uint32(r.record), uint32(r.flags)}
	}
	return kept, keptOffsets, nil
}

// NextOp says which of Collection's writes a batch of NextVersions is.
type NextOp uint32

const (
	NextCreate NextOp = C.HONU_NEXT_CREATE // Collection.Create, collection.go:75-95
	NextUpdate NextOp = C.HONU_NEXT_UPDATE // Collection.Update, collection.go:112-121
	NextMerge  NextOp = C.HONU_NEXT_MERGE  // Collection.Merge, collection.go:123-130
	NextDelete NextOp = C.HONU_NEXT_DELETE // Collection.Delete, collection.go:132-137
)

// Next is one request's answer from NextVersions (honu_next and its key).
type Next struct {
	Version      lamport.Scalar // the assigned version (Assigned)
	Parent       lamport.Scalar // Version.Parent (HasParent)
	ParentRecord uint32         // o.Order of the stored row that is the parent, C.HONU_SEEK_NONE otherwise
	Flags        uint32         // C.HONU_NEXT_*
	Key          keys.Key       // keys.New(id, &Version) when assigned
}

func (n Next) Assigned() bool  { return n.Flags&C.HONU_NEXT_ASSIGNED != 0 }
func (n Next) HasParent() bool { return n.Flags&C.HONU_NEXT_HAS_PARENT != 0 }

// NextVersions decides the version each of a batch of writes writes, which is
// what every write of the store starts with: Store.Drop seeks the stored
// version and calls meta.Tombstone(lamport.ProcessID(), region)
// (store.go:361-395), pid.Next of the stored scalar with that scalar as Parent
// (metadata/collection.go:56-63, lamport/pid.go:10-15); Create starts a history
// at Scalar{PID: 0, VID: 1} (collection.go:87-92). The bodies of
// Collection.Update, Merge and Delete are stubs upstream: op carries out their
// doc comments (collection.go:112-137) with that code, the requests answered
// as the calls would be one after the other (a second Update of an object
// follows the first, a second Delete meets a deleted object). info, the
// decode's record info rows on the device, lets a stored tombstone say "not
// found"; without it every stored object is live. The keys of the assigned
// rows go on to SortKeys and MergeKeys.
//
// UNCOMPILED, like the rest of this file. honu_key_next is exercised on the
// GPU from Python (tests/test_gpu_key_next.py), graph capture included.
func (c *Codec) NextVersions(o *KeyOrder, ids []ulid.ULID, op NextOp, pid lamport.PID, region uint32, now time.Time, info devBuf) ([]Next, error) {
	m := uint64(len(ids))
	if m == 0 {
		return nil, nil
	}
	nextSize := uint64(C.honu_sizeof_next())
	hReq, hOut, hKeys := pinned(uintptr(C.HONU_KEY_LEN*m)), pinned(uintptr(nextSize*m)), pinned(uintptr(C.HONU_KEY_LEN*m))
	defer hReq.free()
	defer hOut.free()
	defer hKeys.free()
	req := hReq.bytes()
	for i, id := range ids {
		copy(req[C.HONU_KEY_LEN*i:], keys.New(id, nil)[:17]) // the ObjectPrefix; the call reads no more
	}
	workBytes := uint64(C.honu_key_next_workspace(C.uint64_t(m)))
	dReq, dOut, dKeys, dSt, work := device(hReq.n), device(hOut.n), device(hKeys.n), device(uintptr(4*m)), device(uintptr(workBytes))
	for _, b := range []devBuf{dReq, dOut, dKeys, dSt, work} {
		defer b.free()
	}
	for _, s := range []C.int32_t{
		C.honu_memcpy_h2d(dReq.p, hReq.p, C.uint64_t(hReq.n), c.stream),
		C.honu_key_next(c.ctx, (*C.uint8_t)(o.sorted.p), (*C.uint64_t)(o.valid.p), C.uint64_t(o.n),
			(*C.uint32_t)(o.order.p), (*C.honu_record_info)(info.p), (*C.uint8_t)(dReq.p), nil, C.uint64_t(m),
			C.uint32_t(op), C.uint32_t(pid), C.uint32_t(region), C.int64_t(now.UnixNano()), (*C.honu_next)(dOut.p),
			(*C.uint8_t)(dKeys.p), (*C.int32_t)(dSt.p), nil, work.p, C.uint64_t(workBytes), c.stream),
		C.honu_memcpy_d2h(hOut.p, dOut.p, C.uint64_t(hOut.n), c.stream),
		C.honu_memcpy_d2h(hKeys.p, dKeys.p, C.uint64_t(hKeys.n), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_key_next", s); err != nil {
			return nil, err
		}
	}
	out := make([]Next, m)
	all := hKeys.bytes()
	for i, r := range unsafe.Slice((*C.honu_next)(hOut.p), m) {
		out[i] = Next{
			Version:      lamport.Scalar{PID: uint32(r.pid), VID: uint64(r.vid)},
			Parent:       lamport.Scalar{PID: uint32(r.parent_pid), VID: uint64(r.parent_vid)},
			ParentRecord: uint32(r.parent_record), Flags: uint32(r.flags),
			Key: append(keys.Key{}, all[C.HONU_KEY_LEN*i:C.HONU_KEY_LEN*(i+1)]...),
		}
	}
	return out, nil
}

// Compared is one object's answer from CompareKeys: a honu_seek row and the
// peer's row.
type Compared struct {
	Seek        // [Pos, End): my versions of the object later than anything the peer holds; Flags also C.HONU_CMP_*
	Peer uint32 // the position of the peer's latest row of the object in its order (C.HONU_SEEK_NONE without PeerHas)
}

func (r Compared) PeerHas() bool  { return r.Flags&C.HONU_CMP_PEER_HAS != 0 }
func (r Compared) Later() bool    { return r.Flags&C.HONU_CMP_LATER != 0 }
func (r Compared) Earlier() bool  { return r.Flags&C.HONU_CMP_EARLIER != 0 }
func (r Compared) Equal() bool    { return r.Flags&C.HONU_CMP_EQUAL != 0 }
func (r Compared) Forked() bool   { return r.PeerHas() && r.Flags&C.HONU_CMP_ANCESTOR == 0 }

// CompareCounts is honu_key_compare's d_counts.
type CompareCounts struct{ Objects, OnlyMine, Later, Earlier, Equal, Forks uint64 }

// CompareKeys decides, for every object of the local order, which side holds
// its later version when two replicas meet: a lamport.Scalar "uses a 'latest
// writer wins' policy to determine how to solve conflicts"
// (lamport/scalar.go:15-24), lamport.Compare is the happens-before test
// (scalar.go:47-78), and bytes.Compare of two keys of one object is
// lamport.Compare of their versions (keys/keys.go:35-36). peer is the order of
// the peer's keys, whole or a digest of one key per object, its latest. One row
// per object of mine, in key order: [Pos, End) are the versions
// latest-writer-wins sends, and the seeks pass to ListKeys and FetchObjects as
// they are. PeerHas without the ancestor bit is a forked write, the branch
// that "can be detected later" (collection.go:77-79); for an Earlier object
// that needs the peer's whole order. The objects only the peer has are the
// rows without PeerHas of CompareKeys(peer, mine). mine is an order that
// SortKeys made (its objects are cut from its key column, as in KeyObjects).
//
// UNCOMPILED, like the rest of this file. honu_key_compare is exercised on the
// GPU from Python (tests/test_gpu_key_compare.py), graph capture included.
func (c *Codec) CompareKeys(mine, peer *KeyOrder) ([]Compared, CompareCounts, error) {
	var counts CompareCounts
	na := mine.n
	workBytes := uint64(C.honu_key_compare_workspace(C.uint64_t(na)))
	dOff, dObjects := device(uintptr(8*(na+1))), device(8)
	dOut, dPeer, dCounts, dWork := device(uintptr(uint64(C.honu_sizeof_seek())*na)), device(uintptr(4*na)), device(64), device(uintptr(workBytes))
	hOut, hPeer, hCounts := pinned(dOut.n), pinned(dPeer.n), pinned(64)
	for _, d := range []devBuf{dOff, dObjects, dOut, dPeer, dCounts, dWork} {
		defer d.free()
	}
	for _, h := range []hostBuf{hOut, hPeer, hCounts} {
		defer h.free()
	}
	for _, s := range []C.int32_t{
		C.honu_key_objects(c.ctx, (*C.uint8_t)(mine.keys.p), (*C.uint32_t)(mine.order.p), (*C.uint64_t)(mine.valid.p),
			C.uint64_t(na), (*C.uint64_t)(dOff.p), nil, (*C.uint64_t)(dObjects.p), mine.work.p,
			C.uint64_t(mine.workBytes), c.stream),
		C.honu_key_compare(c.ctx, (*C.uint8_t)(mine.sorted.p), (*C.uint32_t)(mine.order.p), (*C.uint64_t)(mine.valid.p),
			C.uint64_t(na), (*C.uint64_t)(dOff.p), (*C.uint64_t)(dObjects.p), (*C.uint8_t)(peer.sorted.p),
			(*C.uint64_t)(peer.valid.p), C.uint64_t(peer.n), (*C.honu_seek)(dOut.p), (*C.uint32_t)(dPeer.p),
			(*C.uint64_t)(dCounts.p), dWork.p, C.uint64_t(workBytes), c.stream),
		C.honu_memcpy_d2h(hCounts.p, dCounts.p, 64, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("honu_key_compare", s); err != nil {
			return nil, counts, err
		}
	}
	n := unsafe.Slice((*uint64)(hCounts.p), 8)
	counts = CompareCounts{n[0], n[1], n[2], n[3], n[4], n[5]}
	objects := counts.Objects
	for _, s := range []C.int32_t{ // only what was written: `objects` rows
		C.honu_memcpy_d2h(hOut.p, dOut.p, C.uint64_t(uint64(C.honu_sizeof_seek())*objects), c.stream),
		C.honu_memcpy_d2h(hPeer.p, dPeer.p, C.uint64_t(4*objects), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err := call("download", s); err != nil {
			return nil, counts, err
		}
	}
	rows, at := unsafe.Slice((*C.honu_seek)(hOut.p), objects), unsafe.Slice((*uint32)(hPeer.p), objects)
	out := make([]Compared, objects)
	for j, r := range rows {
		out[j] = Compared{Seek{uint32(r.pos), uint32(r.end), uint32(r.first), uint32(r.latest), uint32(r.flags)}, at[j]}
	}
	return out, counts, nil
}

// Reclaimed is what ReclaimRecords leaves on the device: the per-record state
// of a store over Kept records, and the order of its column over their new
// indices. Values and RecOff are a CSR records arena again; Keys, KeyStatus and
// Info are set where the store's were given.
type Reclaimed struct {
	Kept   uint64   // the records that stay: n and nrec of the calls that follow, b_base of the next merge
	Bytes  uint64   // the bytes of Values
	Source []uint32 // per new record its old index, ascending: for per-record arrays of the caller's own

	Order, Values, RecOff, Keys, KeyStatus, Info devBuf
}

func (r *Reclaimed) Free() {
	for _, d := range []devBuf{r.Order, r.Values, r.RecOff, r.Keys, r.KeyStatus, r.Info} {
		if d.p != nil {
			d.free()
		}
	}
}

// ReclaimRecords frees the space of deleted records: Store.Drop exists "to free
// up space in the database" (store.go:314-322), and after its DeleteBucket
// bbolt "marks the pages as free" (store.go:399-404). o is the column's order
// as SortKeys, MergeKeys or DeleteKeys left it; rec, recOff (nrec + 1 offsets)
// and recBytes are the records arena on the device, keys, keyStatus and info
// the per-record arrays beside it (each may be the zero devBuf). Every record
// that one of the column's valid rows names stays, renumbered in ascending old
// index, so arrival order survives; the others, the removed rows of the
// deletes and the invalid rows of the batches, are freed. The column itself
// stands: its first Kept rows with Reclaimed.Order are the new column. The
// first call sizes (val_cap 0), the second copies into an arena of exactly
// Bytes. The read of Kept is the one host round trip a caller needs before its
// next MergeKeys, whose record base it is.
//
// UNCOMPILED, like the rest of this file. honu_key_reclaim is exercised on the
// GPU from Python (tests/test_gpu_key_reclaim.py, tests/test_gpu_store_reclaim.py),
// graph capture included.
func (c *Codec) ReclaimRecords(o *KeyOrder, rec, recOff devBuf, nrec, recBytes uint64, keys, keyStatus, info devBuf) (out *Reclaimed, err error) {
	n := o.n
	out = &Reclaimed{}
	out.Order, out.RecOff = device(uintptr(4*n)), device(uintptr(8*(nrec+1)))
	if keys.p != nil {
		out.Keys = device(uintptr(C.HONU_KEY_LEN * nrec))
	}
	if keyStatus.p != nil {
		out.KeyStatus = device(uintptr(4 * nrec))
	}
	if info.p != nil {
		out.Info = device(uintptr(uint64(C.honu_sizeof_record_info()) * nrec))
	}
	workBytes := uint64(C.honu_key_reclaim_workspace(C.uint64_t(nrec)))
	work, dSource, dCounts := device(uintptr(workBytes)), device(uintptr(4*nrec)), device(16)
	hSource, hCounts := pinned(uintptr(4*nrec)), pinned(16)
	defer work.free()
	defer dSource.free()
	defer dCounts.free()
	defer hSource.free()
	defer hCounts.free()
	reclaim := func(dValues devBuf, valCap uint64) C.int32_t {
		return C.honu_key_reclaim(c.ctx, (*C.uint32_t)(o.order.p), (*C.uint64_t)(o.valid.p), C.uint64_t(n),
			(*C.uint8_t)(keys.p), (*C.int32_t)(keyStatus.p), (*C.honu_record_info)(info.p),
			(*C.uint8_t)(rec.p), (*C.uint64_t)(recOff.p), C.uint64_t(nrec), C.uint64_t(recBytes), 0,
			(*C.uint32_t)(out.Order.p), nil, (*C.uint32_t)(dSource.p),
			(*C.uint8_t)(out.Keys.p), (*C.int32_t)(out.KeyStatus.p), (*C.honu_record_info)(out.Info.p),
			(*C.uint64_t)(out.RecOff.p), nil, (*C.uint8_t)(dValues.p), C.uint64_t(valCap),
			(*C.uint64_t)(dCounts.p), (*C.uint64_t)(unsafe.Add(dCounts.p, 8)), work.p, C.uint64_t(workBytes), c.stream)
	}
	for _, s := range []C.int32_t{
		reclaim(devBuf{}, 0), // sizes only
		C.honu_memcpy_d2h(hCounts.p, dCounts.p, 16, c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_reclaim", s); err != nil {
			out.Free()
			return nil, err
		}
	}
	out.Kept, out.Bytes = *(*uint64)(hCounts.p), *(*uint64)(unsafe.Add(hCounts.p, 8))
	out.Values = device(uintptr(out.Bytes))
	for _, s := range []C.int32_t{
		reclaim(out.Values, out.Bytes),
		C.honu_memcpy_d2h(hSource.p, dSource.p, C.uint64_t(4*out.Kept), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_reclaim", s); err != nil {
			out.Free()
			return nil, err
		}
	}
	out.Source = append([]uint32(nil), unsafe.Slice((*uint32)(hSource.p), out.Kept)...)
	return out, nil
}

// Routed is what RouteKeys leaves on the device, and the one thing it reads
// back: the offsets. Class c < k is row c of the table of collections, k the
// records of no known collection (the nil bucket of tx.go:117-120), k + 1 the
// positions that do not take part. Rows is a honu_list_row list (range = the
// class), Local the row's index inside its class, Keys the 29-byte keys by
// output row, Bucket the table row per record.
type Routed struct {
	Off   []uint64 // k + 3: the first output row of each class, then m
	Count devBuf   // k + 2 counts on the device: Count + c is MergeKeys' valid count of collection c's segment

	off                        devBuf // Off on the device: off + k is FetchObjects' total of the known collections' rows
	Bucket, Rows, Local, Keys devBuf
}

func (r *Routed) Free() {
	for _, d := range []devBuf{r.Count, r.off, r.Bucket, r.Rows, r.Local, r.Keys} {
		if d.p != nil {
			d.free()
		}
	}
}

// RouteKeys takes a batch apart by collection: the reference store has one
// bbolt bucket per collection, named by the 16-byte collection ID
// (tx.CreateBucketIfNotExists(info.ID[:]), store.go:236-240;
// t.tx.Bucket(collectionID[:]), tx.go:112-120; Tx.Has and Tx.Exists,
// tx.go:141-158), and every object carries its collection (collection.go:86).
// ids holds record i's ID at idStride*i (the decoded rows with their address
// + 112 and stride 352; a packed column with stride 16), status (or the zero
// devBuf) leaves out the records that are not OK, seq (or the zero devBuf) is
// the sequence to keep, SortKeys' order of the batch's keys, so that every
// collection's rows come out in key order; table is the store's k collection
// IDs, ascending and distinct; keys (or the zero devBuf) is gathered by output
// row. The read of Off is the one host round trip a caller needs before the
// per-collection MergeKeys, whose nb and segment pointers are host arguments.
//
// UNCOMPILED, like the rest of this file. honu_key_route is exercised on the
// GPU from Python (tests/test_gpu_key_route.py, tests/test_gpu_store_collections.py),
// graph capture included.
func (c *Codec) RouteKeys(ids devBuf, idStride, m uint64, status, seq, table devBuf, k uint64, keys devBuf) (out *Routed, err error) {
	out = &Routed{}
	out.off, out.Count = device(uintptr(8*(k+3))), device(uintptr(8*(k+2)))
	out.Bucket, out.Rows, out.Local = device(uintptr(4*m)), device(uintptr(uint64(C.honu_sizeof_list_row())*m)), device(uintptr(4*m))
	if keys.p != nil {
		out.Keys = device(uintptr(C.HONU_KEY_LEN * m))
	}
	workBytes := uint64(C.honu_key_route_workspace(C.uint64_t(m)))
	work, hOff := device(uintptr(workBytes)), pinned(uintptr(8*(k+3)))
	defer work.free()
	defer hOff.free()
	for _, s := range []C.int32_t{
		C.honu_key_route(c.ctx, (*C.uint8_t)(ids.p), C.uint64_t(idStride), (*C.int32_t)(status.p), C.uint64_t(m),
			(*C.uint32_t)(seq.p), (*C.uint8_t)(table.p), C.uint64_t(k), (*C.uint8_t)(keys.p),
			(*C.uint32_t)(out.Bucket.p), (*C.honu_list_row)(out.Rows.p), (*C.uint32_t)(out.Local.p), (*C.uint8_t)(out.Keys.p),
			(*C.uint64_t)(out.off.p), (*C.uint64_t)(out.Count.p), work.p, C.uint64_t(workBytes), c.stream),
		C.honu_memcpy_d2h(hOff.p, out.off.p, C.uint64_t(8*(k+3)), c.stream),
		C.honu_stream_sync(c.stream),
	} {
		if err = call("honu_key_route", s); err != nil {
			out.Free()
			return nil, err
		}
	}
	out.Off = append([]uint64(nil), unsafe.Slice((*uint64)(hOff.p), k+3)...)
	return out, nil
}

// Buckets is a bucketed column on the device: k buckets' sorted 29-byte rows
// end to end in one arena of N rows, one uint32 record index per row, k + 1
// uint64 offsets and (optionally) k uint64 counts of valid rows. Bucket c is
// the bucket of row c of the store's sorted table of collections.
type Buckets struct {
	K, N                      uint64 // N: the rows the arena holds, a host bound
	Sorted, Order, Off, Count devBuf
}

func (b *Buckets) Free() {
	for _, d := range []devBuf{b.Sorted, b.Order, b.Off, b.Count} {
		if d.p != nil {
			d.free()
		}
	}
}

// MergeBuckets is collections.Put (store.go:232, 395, 530) for a whole routed
// batch, every record into the bucket tx.Bucket(collectionID[:]) names
// (store.go:236-240, tx.go:112-120): per bucket the stable merge of a's valid
// rows and the rows RouteKeys left for that collection, a's first on equal
// keys, the buckets tight behind each other in a new arena of a.N + m rows. r
// is passed as it stands (Keys the rows, Local the order, its device offsets,
// m the routed batch's positions); base (k uint32 on the device, or the zero
// devBuf with bBase) is added to b's record indices per bucket. Nothing is read
// on the host: the caller that has gone through RouteKeys has paid its read of
// Off already, one that calls honu_key_route itself pays none.
//
// UNCOMPILED, like the rest of this file. honu_key_merge_buckets is exercised
// on the GPU from Python (tests/test_gpu_key_merge_buckets.py,
// tests/test_gpu_store_buckets.py), graph capture included.
func (c *Codec) MergeBuckets(a *Buckets, r *Routed, m uint64, base devBuf, bBase uint32) (*Buckets, error) {
	n := a.N + m
	if n > 0xFFFFFFFF {
		return nil, fmt.Errorf("%d rows: an order indexes at most 2^32 - 1", n)
	}
	o := &Buckets{K: a.K, N: n}
	o.Sorted, o.Order = device(uintptr(C.HONU_KEY_LEN*n)), device(uintptr(4*n))
	o.Off, o.Count = device(uintptr(8*(a.K+1))), device(uintptr(8*a.K))
	s := C.honu_key_merge_buckets(c.ctx, C.uint64_t(a.K), (*C.uint8_t)(a.Sorted.p), (*C.uint32_t)(a.Order.p),
		(*C.uint64_t)(a.Off.p), (*C.uint64_t)(a.Count.p), C.uint64_t(a.N), (*C.uint8_t)(r.Keys.p),
		(*C.uint32_t)(r.Local.p), (*C.uint64_t)(r.off.p), C.uint64_t(m), (*C.uint32_t)(base.p), C.uint32_t(bBase),
		(*C.uint8_t)(o.Sorted.p), (*C.uint32_t)(o.Order.p), (*C.uint64_t)(o.Off.p), (*C.uint64_t)(o.Count.p), c.stream)
	if err := call("honu_key_merge_buckets", s); err != nil {
		o.Free()
		return nil, err
	}
	return o, nil
}

// Has is Collection.Has (collection.go:47-51) for a batch: key != nil &&
// bytes.HasPrefix(key, probe) of the key Seek lands on.
func (c *Codec) Has(o *KeyOrder, probes [][]byte) ([]bool, error) {
	rows, err := c.SeekKeys(o, probes, devBuf{})
	if err != nil {
		return nil, err
	}
	has := make([]bool, len(rows))
	for q, r := range rows {
		has[q] = r.Found()
	}
	return has, nil
}

// Exists is Collection.Exists (collection.go:55-65) for a batch. asWritten
// reads the tombstone of the value at the Seek position, the object's lowest
// version, as the reference's code does (collection.go:57-64); otherwise of the
// latest version, as its comment documents (collection.go:53-54).
func (c *Codec) Exists(o *KeyOrder, probes [][]byte, info devBuf, asWritten bool) ([]bool, error) {
	rows, err := c.SeekKeys(o, probes, info)
	if err != nil {
		return nil, err
	}
	bit := uint32(C.HONU_SEEK_LATEST_LIVE)
	if asWritten {
		bit = C.HONU_SEEK_FIRST_LIVE
	}
	exists := make([]bool, len(rows))
	for q, r := range rows {
		exists[q] = r.Flags&bit != 0
	}
	return exists, nil
}
