"""CPU model of filter_kubernetes' per-record half (plugins/filter_kubernetes/kubernetes.c), restated on the msgpack walker of
tests/modify_model.py: the config map (:905-1320), get_stream (:112-137), value_trim_size (:139-161), merge_log_handler's default
branch (:222-246; flb_pack_json_recs is the JSON oracle the other tests use), pack_map_content (:318-644) and one call (:646-872) --
with the cache entries flb_kube_meta_get would answer a hit with (set_meta: lookup_pod_meta / lookup_namespace_meta and the
properties array of flb_kube_prop_pack) or the pod entry merge_meta_from_tag builds from the tag (set_tag).  The model is the
yardstick of tests/test_kube_*.py and does not use the product."""
import re
import struct

import jsonfuzz
import modify_model as mm

MAX_MERGE_KEY, MAX_ENTRY = 32768, 1 << 20
TAG_PREFIX = b"kube.var.log.containers."
# kube_regex.h:25
KUBE_TAG_TO_REGEX = (r"(?<pod_name>[a-z0-9](?:[-a-z0-9]*[a-z0-9])?(?:\.[a-z0-9](?:[-a-z0-9]*[a-z0-9])?)*)_(?<namespace_name>[^_]+)_"
                     r"(?<container_name>.+)-(?<docker_id>[a-z0-9]{64})\.log$")
TAG_FIELDS = ("pod_name", "namespace_name", "container_name", "docker_id")
_TAG_RX = re.compile(KUBE_TAG_TO_REGEX.replace("(?<", "(?P<").encode())

BOOLS = ("merge_log", "keep_log", "merge_log_trim", "use_tag_for_meta", "use_journal", "dummy_meta", "tls.verify", "tls.verify_hostname", "labels",
         "annotations", "owner_references", "namespace_labels", "namespace_annotations", "namespace_metadata_only", "k8s-logging.parser",
         "k8s-logging.exclude", "cache_use_docker_id", "use_kubelet", "aws_use_pod_association", "use_pod_association",
         "aws_pod_association_host_tls_verify")
OTHERS = ("merge_log_key", "kube_tag_prefix", "merge_parser", "regex_parser", "buffer_size", "tls.debug", "tls.vhost", "kube_url",
          "kube_meta_preload_cache_dir", "kube_ca_file", "kube_ca_path", "kube_namespace_file", "kube_token_file", "kube_token_command", "dns_retries",
          "dns_wait_time", "kubelet_host", "kubelet_port", "kube_token_ttl", "kube_meta_cache_ttl", "kube_meta_namespace_cache_ttl",
          "aws_pod_association_host", "aws_pod_association_endpoint", "aws_pod_association_port", "aws_pod_service_map_ttl",
          "aws_pod_service_map_refresh_interval", "aws_pod_service_preload_cache_dir", "aws_pod_association_host_server_ca_file",
          "aws_pod_association_host_client_cert_file", "aws_pod_association_host_client_key_file", "aws_pod_association_host_tls_debug", "set_platform")
MERGE_UNSET, MERGE_NONE, MERGE_PARSED, MERGE_MAP = -1, 0, 1, 2
NO_STREAM, STDOUT, STDERR, UNKNOWN = 0, 1, 2, 3
JSON_OBJECT = 1                   # root_type of the JSON oracle: an object
# open containers msgpack_unpack_next takes in the stock build (cmake/msgpack.cmake:11 compiles msgpack-c with MSGPACK_EMBED_STACK_SIZE=64;
# the header's own default is 32): the merged map with 63 more open inside a value unpacks again, with 64 it does not
UNPACK_OPEN = 64

_PACK = None


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def pack_json(v):
    """flb_pack_json_recs: (ret, bytes, root_type, records, consumed)"""
    global _PACK
    if _PACK is None:
        _PACK = jsonfuzz.oracle()
    return _PACK(bytes(v))


def utils_bool(v):
    v = v.lower()
    return 1 if v in (b"true", b"on", b"yes") else 0 if v in (b"false", b"off", b"no") else -1


class Config:
    pass


def parse(props):
    """the configuration; ValueError where the filter does not start or create refuses"""
    c = Config()
    c.merge_log, c.keep_log, c.trim, c.merge_log_key, c.prefix, c.tag_meta = False, True, True, None, TAG_PREFIX, False
    seen = set()
    for name, val in props:
        name, val = _b(name).lower().decode("latin-1"), _b(val).split(b"\0")[0]
        if b"${" in val:                                      # the engine would translate it when the property is set
            raise ValueError("environment variables are not translated")
        if name not in BOOLS and name not in OTHERS:
            raise ValueError("unknown property %s" % name)
        if name in seen:                                      # no FLB_CONFIG_MAP_MULT in this map
            raise ValueError("%s is set more than once" % name)
        seen.add(name)
        b = 0
        if name in BOOLS:
            b = utils_bool(val)
            if b < 0:
                raise ValueError("%s: no bool" % name)
        if name in ("merge_parser", "regex_parser"):
            raise ValueError("%s: no parser registry" % name)
        if name in ("use_journal", "dummy_meta") and b:
            raise ValueError("%s is not built" % name)
        if name == "merge_log":
            c.merge_log = bool(b)
        elif name == "keep_log":
            c.keep_log = bool(b)
        elif name == "merge_log_trim":
            c.trim = bool(b)
        elif name == "use_tag_for_meta":
            c.tag_meta = bool(b)
        elif name == "merge_log_key":
            c.merge_log_key = val
        elif name == "kube_tag_prefix":
            c.prefix = val
    if c.merge_log_key is not None and len(c.merge_log_key) >= MAX_MERGE_KEY:
        raise ValueError("merge_log_key too long")
    return c


def describe(c):
    """the text flbgpu_kubernetes_parse_check writes"""
    return "merge_log=%d;keep_log=%d;trim=%d;merge_log_key=%s;tag_meta=%d;prefix=%s" % (
        c.merge_log, c.keep_log, c.trim, c.merge_log_key.hex() if c.merge_log_key is not None else "-", c.tag_meta, c.prefix.hex())


def read_entry(entry, with_props):
    """(the entry's first object, stdout_exclude, stderr_exclude); ValueError where set_meta refuses"""
    if not entry:
        return b"", False, False
    entry = bytes(entry)
    if len(entry) > MAX_ENTRY:
        raise ValueError("an entry over 1 MiB")
    try:
        first = mm.unpack(entry, 0)
    except mm.Bad:
        raise ValueError("the first object does not decode")
    ex = [False, False]
    if with_props and first.end < len(entry):
        try:
            arr = mm.unpack(entry, first.end)
        except mm.Bad:
            raise ValueError("properties of another shape")
        if arr.t != "array" or len(arr.v) != 4 or any(x.t != "bool" for x in arr.v[2:]):
            raise ValueError("properties of another shape")
        for x in arr.v[:2]:
            if x.t == "str":
                raise ValueError("a parser name: no parser registry")
            if x.t != "nil":
                raise ValueError("properties of another shape")
        ex = [x.v for x in arr.v[2:]]
    return entry[:first.end], ex[0], ex[1]


def props_array(stdout_exclude=False, stderr_exclude=False, stdout_parser=None, stderr_parser=None):
    """flb_kube_prop_pack (kube_property.c:252-305)"""
    def p(x):
        return b"\xc0" if x is None else mm.pack_str_hdr(len(x)) + x
    return b"\x94" + p(stdout_parser) + p(stderr_parser) + (b"\xc3" if stdout_exclude else b"\xc2") + (b"\xc3" if stderr_exclude else b"\xc2")


def tag_spans(rest):
    """the named groups of KUBE_TAG_TO_REGEX searched in `rest`: {name: (beg, end)} or None"""
    m = _TAG_RX.search(bytes(rest))
    return {n: m.span(n) for n in TAG_FIELDS} if m else None


def tag_entry(prefix, tag):
    """parse_regex_tag_data's tag branch + merge_meta_from_tag (kube_meta.c:1785-1811, 651-691, 1147-1200): the pod entry or None"""
    tag = bytes(tag)
    if len(prefix) + 1 >= len(tag):
        return None
    rest = tag[len(prefix):]
    sp = tag_spans(rest)
    if sp is None:
        return None
    pairs = [(n, rest[a:b]) for n, (a, b) in ((n, sp[n]) for n in TAG_FIELDS) if b > a]
    return b"\xdf" + struct.pack(">I", len(pairs)) + b"".join(mm.pack_str_hdr(len(k)) + k.encode() + mm.pack_str_hdr(len(v)) + v for k, v in pairs)


def is_word(b, word):
    """strncmp(b, word, len(b)) == 0 for a NUL-terminated word"""
    n = len(b)
    if n <= len(word):
        return word[:n] == b
    return b[:len(word)] == word and b[len(word)] == 0


def get_stream(body):
    """(:112-137) -> (stream, whether the reference reads another member of the union)"""
    for k, v in body.v:
        if k.t == "str" and is_word(k.v, b"stream"):
            if v.t not in ("str", "bin"):
                return UNKNOWN, True
            return (STDOUT if is_word(v.v, b"stdout") else STDERR if is_word(v.v, b"stderr") else UNKNOWN), False
    return NO_STREAM, False


def value_trim_size(s):
    """(:139-161)"""
    size = len(s)
    i = size - 1
    while i > 0:
        if s[i] == 0x0a:
            size -= 1
            i -= 1
            continue
        if s[i - 1] == 0x5c and s[i] in (0x6e, 0x72):
            size -= 2
            i -= 2
        else:
            break
    return size


def low_word_is_3(k):
    if k.t in ("uint", "int"):
        return k.v & 0xffffffff == 3
    if k.t == "f64":
        return struct.unpack(">Q", k.v)[0] & 0xffffffff == 3
    return False


def map32(n):
    return b"\xdf" + struct.pack(">I", n)


class Model:
    """cb_kube_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None); counts() as flbgpu_filter_last_counts; counters()
    as flbgpu_kubernetes_counters (since the model was created, over the calls that answered MODIFIED)"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props):
        self.cfg = parse(props)
        self.pod = self.ns = b""
        self.ex_out = self.ex_err = False
        self.tag_failed = self.cfg.tag_meta
        self.stats = [0, 0, 0, 0]
        self.n_in = self.n_out = 0

    def set_meta(self, pod_entry=None, ns_entry=None):
        pod, eo, ee = read_entry(pod_entry, True)
        ns = read_entry(ns_entry, False)[0]
        self.pod, self.ns, self.ex_out, self.ex_err = pod, ns, eo, ee

    def set_tag(self, tag):
        if not self.cfg.tag_meta:
            raise ValueError("set_tag needs use_tag_for_meta on")
        e = tag_entry(self.cfg.prefix, _b(tag))
        self.tag_failed = e is None
        if e is None:
            return -1
        self.pod, self.ns, self.ex_out, self.ex_err = e, b"", False, False
        return 0

    def tail(self):
        t = b""
        if self.pod:
            t += b"\xaakubernetes" + self.pod
        if self.ns:
            t += b"\xb4kubernetes_namespace" + self.ns
        return t, bool(self.pod) + bool(self.ns)

    def record(self, sec, nsec, body, st):
        """pack_map_content (:318-644): the record's bytes"""
        cfg = self.cfg
        log_index, status, merged = -1, MERGE_UNSET, []
        if cfg.merge_log:
            for i, (k, v) in enumerate(body.v):
                if k.t in ("str", "bin") and k.v == b"log":
                    log_index = i
                    break
                if low_word_is_3(k):
                    st["odd"] = True
        if log_index >= 0:
            v = body.v[log_index][1]
            if v.t == "map":
                status = MERGE_MAP
                merged = [mm.canon(k) + mm.canon(x) for k, x in v.v]
            elif v.t == "str":
                status = MERGE_NONE
                r, packed, rt, nrec, _ = pack_json(v.v)
                if r == 0 and rt == JSON_OBJECT and nrec == 1:
                    status = MERGE_PARSED
                    try:                                      # the packed map is unpacked again, results unchecked (:405-412, :493-496)
                        root = mm.unpack(packed, 0, 32 - UNPACK_OPEN)
                        pairs = root.v if root.t == "map" else []
                    except mm.Bad:
                        pairs = []
                    for k, x in pairs:
                        if x.t == "str" and cfg.trim:
                            n = value_trim_size(x.v)
                            merged.append(mm.canon(k) + mm.pack_str_hdr(n) + x.v[:n])
                        else:
                            merged.append(mm.canon(k) + mm.canon(x))
        ents = []
        for i, (k, v) in enumerate(body.v):
            if i == log_index:
                if cfg.keep_log:
                    if status in (MERGE_NONE, MERGE_PARSED):
                        ents.append(mm.canon(k) + mm.pack_str_hdr(len(v.v)) + v.v)
                        continue
                elif status != MERGE_NONE:
                    continue
            ents.append(mm.canon(k) + mm.canon(v))
        if merged:
            if cfg.merge_log_key is not None:
                ents.append(mm.pack_str_hdr(len(cfg.merge_log_key)) + cfg.merge_log_key + map32(len(merged)) + b"".join(merged))
            else:
                ents += merged
        st["merged"] = status in (MERGE_PARSED, MERGE_MAP)
        tail, npairs = self.tail()
        return b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + map32(0) + map32(len(ents) + npairs) + b"".join(ents) + tail

    def filter(self, data):
        data = bytes(data)
        self.n_in = self.n_out = 0
        if self.tag_failed:                                   # flb_kube_meta_get answered -1 (:700-702)
            return self.NOTOUCH, None
        out, p, n, n_out = bytearray(), 0, 0, 0
        stats = [0, 0, 0]
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                break                                         # the loop ends; what was built goes out (:733, :863-871)
            p = end
            if skip:
                continue
            n += 1
            stream, odd = get_stream(body)
            st = dict(odd=odd, merged=False)
            if ((stream == STDOUT and self.ex_out) or (stream == STDERR and self.ex_err) or
                    (stream in (NO_STREAM, UNKNOWN) and self.ex_out and self.ex_err)):
                stats[1] += 1
                stats[2] += odd
                continue
            if not (0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000):
                return self.NOTOUCH, None                     # set_timestamp refuses (:398-400, :822-834)
            out += self.record(sec, nsec, body, st)
            stats[0] += st["merged"]
            stats[2] += st["odd"]
            n_out += 1
        self.n_in, self.n_out = n, n_out
        for i in range(3):
            self.stats[i] += stats[i]
        return self.MODIFIED, bytes(out)

    def counts(self):
        return self.n_in, self.n_out

    def counters(self):
        return tuple(self.stats)
