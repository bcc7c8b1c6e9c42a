"""Ordered delivery for a request whose text chunks run in parallel rows (`batching.py`; pure Python, nothing here touches
torch, the engine or the GPU).

The chunks of one request are independent and may run side by side, but the consumer must receive what the serial run would
have produced: every item of chunk 0, then every item of chunk 1, and so on, then one `None`.  `ChunkOrder` takes the items
as the rows produce them, in any interleaving, and forwards them in that order:

  * items of the chunk at the head (the lowest chunk that has not finished) pass straight through;
  * items of a later chunk are held; when every chunk before it has finished they are flushed in arrival order, and the
    chunk is the head from then on;
  * the single `None` follows the last chunk's `finish`;
  * after `cancel` nothing is forwarded any more, and the `None` is emitted at once (once).
"""

from __future__ import annotations


class ChunkOrder:
    """`emit(item)` receives the ordered sequence and a final `emit(None)`; `chunks` is the number of text chunks."""

    __slots__ = ("emit", "chunks", "head", "held", "finished", "closed")

    def __init__(self, chunks: int, emit):
        if chunks < 1:
            raise ValueError("a request has at least one chunk")
        self.emit, self.chunks = emit, int(chunks)
        self.head = 0            # the chunk whose items pass through
        self.held: dict = {}     # chunk index -> items that wait for the chunks before it
        self.finished = set()    # chunks past the head that have finished
        self.closed = False      # the sentinel has been emitted

    def push(self, chunk: int, item):
        if self.closed:
            return
        if not self.head <= chunk < self.chunks:
            raise ValueError(f"chunk {chunk} is not one of the open chunks [{self.head}, {self.chunks})")
        if chunk in self.finished:
            raise ValueError(f"chunk {chunk} has finished")
        if chunk == self.head:
            self.emit(item)
        else:
            self.held.setdefault(chunk, []).append(item)

    def finish(self, chunk: int):
        if self.closed:
            return
        if not self.head <= chunk < self.chunks or chunk in self.finished:
            raise ValueError(f"chunk {chunk} is not open")
        self.finished.add(chunk)
        while self.head in self.finished:
            self.finished.discard(self.head)
            self.head += 1
            for item in self.held.pop(self.head, ()):
                self.emit(item)
        if self.head == self.chunks:
            self.closed = True
            self.emit(None)

    def cancel(self):
        """drops what is held; the consumer's sequence ends here"""
        if self.closed:
            return
        self.closed = True
        self.held.clear()
        self.emit(None)
